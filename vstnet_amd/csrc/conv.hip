// 3x3 reflect-padded convolutions of the coupling blocks: the kernels, their launches and the block runner (whole passes:
// revnet.hip).
//
// Reference semantics (paths relative to the reference root):
//   residual_block.conv     models/RevResNet.py:79-88   ReflectionPad2d(1)+Conv2d(3x3,bias) x3, ReLU between
//   residual_block.forward  models/RevResNet.py:96-104  (x1,x2) -> (x2, F(x2)+x1)   [stride 2: squeeze both]
//   residual_block.inverse  models/RevResNet.py:106-116 (x2,y1) -> (y1-F(x2), x2)
//   RevResNet._forward/_inverse  models/RevResNet.py:210-239, channel_reduction :131-163
//
// Every conv is an implicit GEMM  D[pixel][co] = sum_{tap,ci} A[pixel+tap][ci] * W[tap][ci][co]
// on v_mfma_f32_16x16x32_bf16 with split operands: a = a_hi + a_lo, w = w_hi + w_lo (bf16 each),
// D += a_hi*w_hi + a_lo*w_hi + a_hi*w_lo, fp32 accumulate (error ~2^-17 per product; the state in
// HBM stays fp32).  A workgroup (4 waves) owns a 16-wide x (4*MR)-high tile of output pixels and
// NT output channels; activations are staged fp32 -> {hi,lo} bf16 into an LDS image
// [channel-group of 8][slot][8 x bf16] in which the 16 pixels of an MFMA row block are consecutive
// 16-byte slots (bank-conflict-free ds_read_b128 for every tap shift); weights are pre-packed in
// fragment order (layout.hip) and copied straight into LDS.
#include "common.h"

struct ConvArgs {
    const float* in;
    float* out;
    const unsigned char* packed;
    const float* bias;
    int Hin, Win, Hout, Wout;
    int Wq;                      // W/4 of the full image (state addressing)
    size_t in_img_stride;        // floats per image
    size_t out_img_stride;
    float sign;                  // OUT_STATE: out += sign * (conv + bias)
    int tiles_x, tiles_y, tiles_total;   // 1-D grid of round_up(tiles_total, 8) workgroups, see xcd_tile()
    const unsigned char* packed1;        // conv_pair_kernel: conv.4's packed weights and bias (in = h1)
    const float* bias1;
    unsigned char* out_sp;               // OUT_SP: the output goes to split fp16 planes (common.h) instead of `out`
    size_t out_sp_img_bytes;
    unsigned trace_base;                 // -DVST_TRACE=3 builds: first record of this launch in the trace buffer
    float* rgb;                          // conv_pair_kernel<..., OUT_RGB>: the image x[B][rgb_c][H][W] (or null) ...
    unsigned char* rgb_u8;               // ... or the HWC uint8 frames [B][H][W][3] that the last inverse block writes
    int rgb_c;                           // channels of `rgb` (<= 16)
};

// Workgroups are dispatched round-robin over the 8 XCDs, each with its own L2.  Give XCD k the contiguous
// (row-major) range of tiles [k*per, (k+1)*per) so that tiles sharing a halo also share an L2.
#ifdef VST_TRACE
// Diagnostic builds only (-DVST_TRACE=1: conv_pair_kernel, 2: conv_mfma_kernel): every workgroup of the LAST traced launch
// leaves {start, end (100 MHz ticks), HW_ID, XCC_ID} here; tools/trace_grid.py reads them back through vst_trace_dump.
// -DVST_TRACE=3: EVERY workgroup of EVERY conv launch (classes 1, 2, 4 = conv_pipe_kernel) appends
// {start, end, HW_ID | XCC_ID << 32, class | Cin << 8 | Cout << 20 | blockIdx << 32} to a caller-provided buffer
// (vst_trace_set; tools/trace_cu.py): which kernels of which streams were resident on which CU, when.
__device__ unsigned long long vst_trace_buf[4 * 16384];
__device__ unsigned long long* vst_trace_ptr;
__device__ unsigned vst_trace_cap;
static std::atomic<unsigned> vst_trace_host_n{0};     // next free record (launch sites reserve one per workgroup)
#define VST_TRACE_RESERVE(t_, grid_) (t_).trace_base = vst_trace_host_n.fetch_add((unsigned)(grid_));
#define VST_TRACE_BEGIN(which)                                                                                  \
    const unsigned long long trace_t0 = __builtin_amdgcn_s_memrealtime();   /* scalar: no VGPR is held for it */
#define VST_TRACE_END_(which, cin_, cout_)                                                                      \
    if (VST_TRACE == (which) || VST_TRACE == 3) {                                                               \
        __builtin_amdgcn_s_waitcnt(0);                                                                          \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                       \
        if (threadIdx.x == 0 && (VST_TRACE == 3 || blockIdx.x < 16384)) {                                       \
            unsigned hw, xcc;                                                                                   \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                    \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                                  \
            if (VST_TRACE == 3) {                                                                               \
                const unsigned i_ = a.trace_base + blockIdx.x;                                                  \
                if (vst_trace_ptr && i_ < vst_trace_cap) {                                                      \
                    unsigned long long* r_ = vst_trace_ptr + 4 * (size_t)i_;                                    \
                    r_[0] = trace_t0;                                                                           \
                    r_[1] = __builtin_amdgcn_s_memrealtime();                                                   \
                    r_[2] = hw | ((unsigned long long)xcc << 32);                                               \
                    r_[3] = (which) | ((cin_) << 8) | ((cout_) << 20) | ((unsigned long long)blockIdx.x << 32); \
                }                                                                                               \
            } else {                                                                                            \
                vst_trace_buf[4 * blockIdx.x + 0] = trace_t0;                                                   \
                vst_trace_buf[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();                           \
                vst_trace_buf[4 * blockIdx.x + 2] = hw;                                                         \
                vst_trace_buf[4 * blockIdx.x + 3] = xcc;                                                        \
            }                                                                                                   \
        }                                                                                                       \
    }
#define VST_TRACE_END(which) VST_TRACE_END_(which, 0, 0)
extern "C" __attribute__((visibility("default"))) int vst_trace_dump(unsigned long long* host, int n_wg) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vst_trace_buf), sizeof(unsigned long long) * 4 * (size_t)n_wg);
}
// append mode: records go to `dev_buf` (cap records of 4 x u64); returns the number of records written so far through *n
extern "C" __attribute__((visibility("default"))) int vst_trace_set(unsigned long long* dev_buf, unsigned cap) {
    const unsigned zero = 0;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(vst_trace_ptr), &dev_buf, sizeof(dev_buf));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(vst_trace_cap), &cap, sizeof(cap));
    (void)zero;
    vst_trace_host_n.store(0);
    return (int)e;
}
extern "C" __attribute__((visibility("default"))) int vst_trace_count(unsigned* n) { *n = vst_trace_host_n.load(); return 0; }
#else
#define VST_TRACE_BEGIN(which)
#define VST_TRACE_END(which)
#define VST_TRACE_END_(which, cin_, cout_)
#define VST_TRACE_RESERVE(t_, grid_)
#endif

__device__ __forceinline__ bool xcd_tile(const ConvArgs& a, int& bx, int& by, int& bz) {
    const int g = blockIdx.x, per = gridDim.x >> 3;
    const int n = (g & 7) * per + (g >> 3);
    if (n >= a.tiles_total) return false;
    bx = n % a.tiles_x;
    const int r = n / a.tiles_x;
    by = r % a.tiles_y;
    bz = r / a.tiles_y;
    return true;
}

template <int CIN, int COUT, int STRIDE, int MRO = 0, int KSO = 0>   // MRO: tile rows per wave if not the default; KSO: k steps
struct ConvCfg {
    static constexpr int NT = COUT >= 64 ? 64 : 16;      // output channels per workgroup
    static constexpr int NB = NT / 16;                   // 16-wide N blocks per wave
    static constexpr int COUTP = (COUT + 15) / 16 * 16;
    static constexpr int NCOT = COUTP / NT;              // co tiles (grid.z factor)
    static constexpr int MR = MRO ? MRO : (STRIDE == 2 ? 2 : 4);   // tile rows (16-pixel M blocks) per wave
    static constexpr int TH = 4 * MR, TW = 16;
    static constexpr int IH = (TH - 1) * STRIDE + 3, IW = (TW - 1) * STRIDE + 3;
    static constexpr int NSLOT = (IH * IW + 15) / 16 * 16;
    static constexpr int CC = CIN >= 32 ? 32 : CIN;      // input channels staged per chunk
    static constexpr int NCHUNK = CIN / CC;
    static constexpr int CIG = CC >= 8 ? CC / 8 : 1;     // 8-channel groups per chunk
    static constexpr int KS = KSO ? KSO : (CIN >= 32 ? 9 : (CIN == 16 ? 5 : 2));   // 32-deep k steps per chunk
    static constexpr int A_PLANE = CIN == 4 ? NSLOT * 8 : CIG * NSLOT * 16;
    static constexpr int B_PLANE = KS * 4 * NT * 16;
    static constexpr int LDS_BYTES = 2 * A_PLANE + 2 * B_PLANE;
    static constexpr int LDS_BYTES_T2 = 2 * A_PLANE + B_PLANE;     // TERMS == 2: one weight plane
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// TERMS == 3: bf16 hi / lo (3-term product with split weights); TERMS == 2: fp16 hi / lo (2-term product w_hi (x_hi + x_lo),
// the arithmetic of conv3.hip; values saturate at +-65504 in the hi part)
__device__ __forceinline__ void split8_f16(const float4 v0, const float4 v1, uint4& hi, uint4& lo, float& amax) {
    const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    u32x4 h, l;
    split8_sp(f, h, l, amax);
    hi = __builtin_bit_cast(uint4, h);
    lo = __builtin_bit_cast(uint4, l);
}

__device__ __forceinline__ void split4_f16(const float4 v, uint2& hi, uint2& lo, float& amax) {
    const float f[4] = {v.x, v.y, v.z, v.w};
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    f16x4 h, l;
#ifndef VST_NO_RANGE_CHECK
    amax = fmaxf(fmaxf(amax, fabsf(f[0])), fmaxf(fmaxf(fabsf(f[1]), fabsf(f[2])), fabsf(f[3])));
#endif
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float c = __builtin_amdgcn_fmed3f(f[i], -65504.f, 65504.f);
        h[i] = (_Float16)c;
        l[i] = (_Float16)(f[i] - (float)h[i]);
    }
    hi = __builtin_bit_cast(uint2, h);
    lo = __builtin_bit_cast(uint2, l);
}

__device__ __forceinline__ void split8(const float4 v0, const float4 v1, uint4& hi, uint4& lo) {
    const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    bf16x8 h, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = (__bf16)f[i];
        l[i] = (__bf16)(f[i] - (float)h[i]);
    }
    hi = __builtin_bit_cast(uint4, h);
    lo = __builtin_bit_cast(uint4, l);
}

__device__ __forceinline__ void split4(const float4 v, uint2& hi, uint2& lo) {
    const float f[4] = {v.x, v.y, v.z, v.w};
    bf16x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = (__bf16)f[i];
        l[i] = (__bf16)(f[i] - (float)h[i]);
    }
    hi = __builtin_bit_cast(uint2, h);
    lo = __builtin_bit_cast(uint2, l);
}

// ---- register epilogue ---------------------------------------------------------------------------
// The MFMAs are issued as D = W * X^T (weights are the A operand, pixels the B operand), so lane
// (lrow, kg) ends up with D[co = 4*kg + r][pixel = lrow]: four CONSECUTIVE channels of one pixel per
// accumulator -> one float4 store (or float4 read-modify-write of the state) per 16x16 tile, no LDS.
template <int COUT, int NB>
__device__ __forceinline__ void load_bias(const ConvArgs& a, int co_lane, float4 (&bias)[NB]) {
#pragma unroll
    for (int n = 0; n < NB; ++n)
        bias[n] = co_lane + n * 16 < COUT ? *(const float4*)(a.bias + co_lane + n * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// address of the 4 channels [co_lane + 16 n, +4) of output pixel (oy, ox); nullptr when outside the image / channel range
template <int COUT, bool OUT_STATE, bool FULL = false>
__device__ __forceinline__ float4* out_ptr(const ConvArgs& a, float* out_img, int oy, int ox, int co) {
    if (!FULL && (oy >= a.Hout || ox >= a.Wout || co >= COUT)) return nullptr;
    if (OUT_STATE) return (float4*)(out_img + zc_offset(vst_level_of_channels(COUT), oy, ox, a.Wq) + co);
    return (float4*)(out_img + ((size_t)oy * a.Wout + ox) * COUT + co);
}

template <int COUT, int MR, int NB, bool FULL = false>
__device__ __forceinline__ void load_old(const ConvArgs& a, float* out_img, int oy0, int ox, int co_lane,
                                         float4 (&old)[MR][NB]) {
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const float4* p = out_ptr<COUT, true, FULL>(a, out_img, oy0 + m, ox, co_lane + n * 16);
            old[m][n] = (FULL || p) ? *p : make_float4(0.f, 0.f, 0.f, 0.f);
        }
}

// OUT_STATE: out = old + sign * (acc + bias);  else: out = relu(acc + bias)
template <int COUT, bool OUT_STATE, int MR, int NB, bool FULL = false>
__device__ __forceinline__ void store_tile(const ConvArgs& a, float* out_img, int oy0, int ox, int co_lane,
                                           const f32x4 (&acc)[MR][NB], const float4 (&bias)[NB],
                                           const float4 (&old)[MR][NB]) {
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            float4* p = out_ptr<COUT, OUT_STATE, FULL>(a, out_img, oy0 + m, ox, co_lane + n * 16);
            if (!FULL && !p) continue;
            float4 r = make_float4(acc[m][n][0] + bias[n].x, acc[m][n][1] + bias[n].y, acc[m][n][2] + bias[n].z,
                                   acc[m][n][3] + bias[n].w);
            if (OUT_STATE) {
                const float4 o = old[m][n];
                r = make_float4(o.x + a.sign * r.x, o.y + a.sign * r.y, o.z + a.sign * r.z, o.w + a.sign * r.w);
            } else {
                r.x = r.x > 0.f ? r.x : 0.f; r.y = r.y > 0.f ? r.y : 0.f;
                r.z = r.z > 0.f ? r.z : 0.f; r.w = r.w > 0.f ? r.w : 0.f;
            }
            *p = r;
        }
}

#define MFMA3(acc, wh, wl, xh, xl)                                              \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc, 0, 0, 0)

// the same with the number of terms chosen at compile time: operands are 16-byte containers (bf16x8), read as fp16 when TERMS == 2
#define MFMA_T(acc, wh, wl, xh, xl)                                                                                          \
    if constexpr (TERMS == 3) {                                                                                               \
        MFMA3(acc, wh, wl, xh, xl);                                                                                           \
    } else {                                                                                                                  \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xl), acc, 0, 0, 0); \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0); \
    }
// (range_amax: the kernel's running max |x| of what it rounds to fp16, handed to vst_note_range once at its end)
#define SPLIT8_T(v0_, v1_, h_, l_) { if constexpr (TERMS == 3) split8(v0_, v1_, h_, l_); else split8_f16(v0_, v1_, h_, l_, range_amax); }
#define SPLIT4_T(v_, h_, l_) { if constexpr (TERMS == 3) split4(v_, h_, l_); else split4_f16(v_, h_, l_, range_amax); }

// ---- generic kernel: one tile per workgroup, staging per input-channel chunk (all shapes) --------------
// OUT_H16 (an intermediate h1, not the state): ReLU(acc + bias) is written as fp16, channels-last like the fp32 form
// (VST_PREC_F16X2H: the pair kernel reads h1 as the fp16 operand it is, one MFMA per product in conv.4)
//
// FOLD (the 16 -> 4 conv.1 of the stage-1 blocks, bf16x3): the horizontal tap goes into the weight operand's rows instead of K.
// Row (tx, co) = 4 tx + co fills 12 of the 16 rows that COUT = 4 leaves three quarters empty, K = (ty, ci) = 48 -> two k steps
// instead of five.  The pixel operand is the same LDS image read at the UN-shifted pixel, so D[(tx, co)][q] is wanted for every
// image column, ring included: a wave's 4 rows x 18 columns are linearised (q = 18 r + c, which is also the slot step of the
// image, IW = 18) into five 16-pixel blocks - 30 MFMAs per wave instead of 60.  out[co][r][x] = sum_tx D[(tx, co)][18 r + x + tx]
// is a shift-add across pixel columns: the accumulators go through the (then dead) image region of LDS, [q][tx][co] per wave,
// and lane (x, r) adds its three float4 in the fixed order (tx0 + tx1) + tx2.  The fragments are a permutation of the packed
// ones ((ks, kg, row) <- the 16-byte item of tap 3 ty + tx, channel group kg & 1, row co), gathered at staging time: the packed
// layout does not change.
template <int CIN, int COUT, int STRIDE, bool IN_STATE, bool OUT_STATE, bool OUT_SP = false, int TERMS = 3, bool OUT_H16 = false,
          bool FOLD = false>
__global__ __launch_bounds__(256) void conv_mfma_kernel(const ConvArgs a) {
    static_assert(!FOLD || (CIN == 16 && COUT == 4 && STRIDE == 1 && TERMS == 3 && !OUT_STATE && !OUT_SP && !OUT_H16),
                  "tap-folded form: conv.1 of the 16-channel blocks, bf16x3");
    using C = ConvCfg<CIN, COUT, STRIDE, 0, FOLD ? 2 : 0>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const a_hi = smem;
    unsigned char* const a_lo = smem + C::A_PLANE;
    unsigned char* const b_hi = smem + 2 * C::A_PLANE;
    unsigned char* const b_lo = TERMS == 3 ? b_hi + C::B_PLANE : b_hi;     // TERMS == 2: one weight plane

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 15, kg = lane >> 4;
    int bx, by, bz;
    if (!xcd_tile(a, bx, by, bz)) return;
    float range_amax = 0.f;
    VST_TRACE_BEGIN(2)
    const int tx0 = bx * C::TW, ty0 = by * C::TH;
    const int b = bz / C::NCOT, co0 = (bz % C::NCOT) * C::NT;

    const float* const in_img = a.in + (size_t)b * a.in_img_stride;
    const PackedConvLayout PL = packed_conv_layout(COUT, CIN);
    const unsigned char* const w_hi = a.packed + (TERMS == 3 ? PL.f32_bytes : PL.f16_offset);
    const unsigned char* const w_lo = w_hi + PL.frag_bytes;                 // (not read when TERMS == 2)

    f32x4 acc[C::MR][C::NB];
#pragma unroll
    for (int m = 0; m < C::MR; ++m)
#pragma unroll
        for (int n = 0; n < C::NB; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-lane slot of tile row (wave*MR), pixel lrow, tap (0,0)
    const int slot_base = (wave * C::MR * STRIDE) * C::IW + lrow * STRIDE;

    // Staging is split into "fetch" (global -> registers) and "land" (bf16 split, registers -> LDS) so that the
    // latencies overlap: weights and activations of a chunk are fetched together, the next chunk is fetched before this
    // chunk's MFMAs, and the read-modify-write state values are fetched before the last chunk's MFMAs wherever they
    // fit in registers that are dead until the epilogue (s_memtime stamps of the synchronous form showed the weight
    // fetch, the second chunk's fetch and the old-state fetch as 2-2.5 us waits each in a 13 us workgroup).
    constexpr int A_ITEMS_T = CIN == 4 ? C::IH * C::IW : C::IH * C::IW * C::CIG;
    constexpr int AIT = (A_ITEMS_T + 255) / 256, NV = CIN == 4 ? 1 : 2;
    constexpr int W_ITEMS_T = C::KS * 4 * C::NT, WIT = (W_ITEMS_T + 255) / 256;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // native vectors: these arrays must stay in VGPRs
    f32x4 areg[AIT][NV];
    u32x4 wreg[WIT][2];
#define F4(v_) make_float4((v_)[0], (v_)[1], (v_)[2], (v_)[3])
#define GEN_FETCH(chunk_)                                                                           \
    _Pragma("unroll") for (int it = 0; it < WIT; ++it) {                                           \
        int idx = it * 256 + tid;                                                                  \
        idx = idx < W_ITEMS_T ? idx : W_ITEMS_T - 1;                                               \
        const int co = idx % C::NT, r = idx / C::NT;                                               \
        if constexpr (FOLD) {                                                                      \
            const int ty = 2 * (r >> 2) + ((r >> 1) & 1), tx = co >> 2;      /* r = 4 ks + kg */     \
            const bool live = ty < 3 && tx < 3;                                                    \
            const int tap = live ? 3 * ty + tx : 0;                                                \
            const size_t src = ((size_t)((tap >> 1) * 4 + (tap & 1) * 2 + (r & 1)) * 16 + (co & 3)) * 16; \
            const u32x4 h_ = *(const u32x4*)(w_hi + src), l_ = *(const u32x4*)(w_lo + src);        \
            wreg[it][0] = live ? h_ : u32x4{0u, 0u, 0u, 0u};                                       \
            wreg[it][1] = live ? l_ : u32x4{0u, 0u, 0u, 0u};                                       \
        } else {                                                                                   \
            const size_t src = ((size_t)((chunk_) * C::KS * 4 + r) * C::COUTP + co0 + co) * 16;    \
            wreg[it][0] = *(const u32x4*)(w_hi + src);                                             \
            if (TERMS == 3) wreg[it][1] = *(const u32x4*)(w_lo + src);                             \
        }                                                                                          \
    }                                                                                              \
    _Pragma("unroll") for (int it = 0; it < AIT; ++it) {                                           \
        int idx = it * 256 + tid;                                                                  \
        idx = idx < A_ITEMS_T ? idx : A_ITEMS_T - 1;                                               \
        const int cig = CIN == 4 ? 0 : idx % C::CIG, slot = CIN == 4 ? idx : idx / C::CIG;         \
        const int iy = slot / C::IW, ix = slot - iy * C::IW;                                       \
        const int gy = reflect_clamp(ty0 * STRIDE - 1 + iy, a.Hin);                                \
        const int gx = reflect_clamp(tx0 * STRIDE - 1 + ix, a.Win);                                \
        const size_t off = IN_STATE ? zc_offset(vst_level_of_channels(CIN), gy, gx, a.Wq)          \
                                    : ((size_t)gy * a.Win + gx) * CIN;                             \
        const float* p = in_img + off + (chunk_) * C::CC + cig * 8;                                \
        areg[it][0] = *(const f32x4*)p;                                                            \
        if (NV == 2) areg[it][NV - 1] = *(const f32x4*)(p + 4);                                    \
    }
    // threads past the end repeat the last item (same value to the same address): no predicates, so the compiler keeps
    // every fetch where it was issued
#define GEN_LAND()                                                                                 \
    _Pragma("unroll") for (int it = 0; it < AIT; ++it) {                                           \
        int idx = it * 256 + tid;                                                                  \
        idx = idx < A_ITEMS_T ? idx : A_ITEMS_T - 1;                                               \
        if (CIN == 4) {                                                                            \
            uint2 h, l;                                                                            \
            SPLIT4_T(F4(areg[it][0]), h, l);                                                       \
            *(uint2*)(a_hi + idx * 8) = h;                                                         \
            *(uint2*)(a_lo + idx * 8) = l;                                                         \
        } else {                                                                                   \
            const int cig = idx % C::CIG, slot = idx / C::CIG;                                     \
            uint4 h, l;                                                                            \
            SPLIT8_T(F4(areg[it][0]), F4(areg[it][NV - 1]), h, l);                                 \
            *(uint4*)(a_hi + (cig * C::NSLOT + slot) * 16) = h;                                    \
            *(uint4*)(a_lo + (cig * C::NSLOT + slot) * 16) = l;                                    \
        }                                                                                          \
    }                                                                                              \
    _Pragma("unroll") for (int it = 0; it < WIT; ++it) {                                           \
        int idx = it * 256 + tid;                                                                  \
        idx = idx < W_ITEMS_T ? idx : W_ITEMS_T - 1;                                               \
        *(u32x4*)(b_hi + idx * 16) = wreg[it][0];                                                  \
        if (TERMS == 3) *(u32x4*)(b_lo + idx * 16) = wreg[it][1];                                  \
    }

    float* const out_img = a.out + (size_t)b * a.out_img_stride;
    float4 bias[C::NB], old[C::MR][C::NB];
    const bool interior = COUT % 16 == 0 && ty0 + C::TH <= a.Hout && tx0 + C::TW <= a.Wout;   // no predicates needed
    // fetch the old state before the MFMAs only where its registers are free anyway (big register tiles: the 16-value
    // tiles of the 4->16 conv lose more to occupancy than they gain)
    constexpr bool EARLY_OLD = OUT_STATE && C::MR * C::NB >= 16;
    auto fetch_old = [&]() __attribute__((always_inline)) {
        if (interior) load_old<COUT, C::MR, C::NB, true>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, co0 + 4 * kg, old);
        else load_old<COUT, C::MR, C::NB>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, co0 + 4 * kg, old);
    };

    GEN_FETCH(0);
    GEN_LAND();
    if constexpr (FOLD) {
        constexpr int NPX = C::MR * C::IW, NBLK = (NPX + 15) / 16;       // 72 region pixels of the wave in 5 blocks
        static_assert(4 * NBLK * 16 * 12 * 4 <= 2 * C::A_PLANE, "the transposed accumulators fit the image region");
        __syncthreads();
        f32x4 facc[NBLK];
#pragma unroll
        for (int j = 0; j < NBLK; ++j) facc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const int boff = ((ks * 4 + kg) * 16 + lrow) * 16;
            const bf16x8 wh = __builtin_bit_cast(bf16x8, *(const uint4*)(b_hi + boff));
            const bf16x8 wl = __builtin_bit_cast(bf16x8, *(const uint4*)(b_lo + boff));
            int ty = 2 * ks + (kg >> 1);
            ty = ty > 2 ? 2 : ty;                                       // (tap row 3: zero weights, any written slot)
#pragma unroll
            for (int j = 0; j < NBLK; ++j) {
                int q = j * 16 + lrow;
                q = q < NPX ? q : NPX - 1;                               // (the last block's tail: computed, never read back)
                const int aoff = ((kg & 1) * C::NSLOT + (wave * C::MR + ty) * C::IW + q) * 16;
                const bf16x8 xh = __builtin_bit_cast(bf16x8, *(const uint4*)(a_hi + aoff));
                const bf16x8 xl = __builtin_bit_cast(bf16x8, *(const uint4*)(a_lo + aoff));
                MFMA3(facc[j], wh, wl, xh, xl);
            }
        }
        __syncthreads();                                                 // every wave is done with the image
        float* const sc = (float*)smem + wave * (NBLK * 16 * 12);       // [q][tx][co] of this wave
        if (kg < 3) {
#pragma unroll
            for (int j = 0; j < NBLK; ++j) *(f32x4*)(sc + ((j * 16 + lrow) * 3 + kg) * 4) = facc[j];
        }
        __syncthreads();
        const int q0 = kg * C::IW + lrow;                                // lane (x = lrow, r = kg): one output pixel
        const f32x4 d0 = *(const f32x4*)(sc + ((q0 + 0) * 3 + 0) * 4);
        const f32x4 d1 = *(const f32x4*)(sc + ((q0 + 1) * 3 + 1) * 4);
        const f32x4 d2 = *(const f32x4*)(sc + ((q0 + 2) * 3 + 2) * 4);
        const float4 bs = *(const float4*)a.bias;
        const int oy = ty0 + wave * C::MR + kg, ox = tx0 + lrow;
        if (oy < a.Hout && ox < a.Wout) {
            float4 r = make_float4((d0[0] + d1[0]) + d2[0] + bs.x, (d0[1] + d1[1]) + d2[1] + bs.y,
                                   (d0[2] + d1[2]) + d2[2] + bs.z, (d0[3] + d1[3]) + d2[3] + bs.w);
            r.x = r.x > 0.f ? r.x : 0.f; r.y = r.y > 0.f ? r.y : 0.f;
            r.z = r.z > 0.f ? r.z : 0.f; r.w = r.w > 0.f ? r.w : 0.f;
            *(float4*)(a.out + (size_t)b * a.out_img_stride + ((size_t)oy * a.Wout + ox) * COUT) = r;
        }
        VST_TRACE_END_(2, CIN, COUT)
        return;
    }
#pragma unroll
    for (int chunk = 0; chunk < C::NCHUNK; ++chunk) {
        __syncthreads();
        if (chunk + 1 < C::NCHUNK) { GEN_FETCH(chunk + 1); }
        if (EARLY_OLD && chunk == C::NCHUNK - 1) fetch_old();

        // ---- MFMA over the chunk's k steps ---------------------------------------------------------
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            bf16x8 wh[C::NB], wl[C::NB];
#pragma unroll
            for (int n = 0; n < C::NB; ++n) {
                const int boff = ((ks * 4 + kg) * C::NT + n * 16 + lrow) * 16;
                wh[n] = __builtin_bit_cast(bf16x8, *(const uint4*)(b_hi + boff));
                if (TERMS == 3) wl[n] = __builtin_bit_cast(bf16x8, *(const uint4*)(b_lo + boff)); else wl[n] = wh[n];
            }
#pragma unroll
            for (int m = 0; m < C::MR; ++m) {
                bf16x8 xh, xl;
                if (CIN >= 32) {
                    const int dy = ks / 3, dx = ks - dy * 3;
                    const int slot = slot_base + (m * STRIDE + dy) * C::IW + dx;
                    const int aoff = (kg * C::NSLOT + slot) * 16;
                    xh = __builtin_bit_cast(bf16x8, *(const uint4*)(a_hi + aoff));
                    xl = __builtin_bit_cast(bf16x8, *(const uint4*)(a_lo + aoff));
                } else if (CIN == 16) {
                    int tap = 2 * ks + (kg >> 1);
                    tap = tap > 8 ? 8 : tap;
                    const int dy = tap / 3, dx = tap - dy * 3;
                    const int slot = slot_base + (m * STRIDE + dy) * C::IW + dx;
                    const int aoff = ((kg & 1) * C::NSLOT + slot) * 16;
                    xh = __builtin_bit_cast(bf16x8, *(const uint4*)(a_hi + aoff));
                    xl = __builtin_bit_cast(bf16x8, *(const uint4*)(a_lo + aoff));
                } else {
                    int t0 = 8 * ks + 2 * kg;
                    t0 = t0 > 8 ? 8 : t0;
                    const int t1 = t0 + 1 > 8 ? 8 : t0 + 1;
                    const int s0 = slot_base + (m * STRIDE + t0 / 3) * C::IW + t0 % 3;
                    const int s1 = slot_base + (m * STRIDE + t1 / 3) * C::IW + t1 % 3;
                    const uint2 h0 = *(const uint2*)(a_hi + s0 * 8), h1 = *(const uint2*)(a_hi + s1 * 8);
                    const uint2 l0 = *(const uint2*)(a_lo + s0 * 8), l1 = *(const uint2*)(a_lo + s1 * 8);
                    xh = __builtin_bit_cast(bf16x8, make_uint4(h0.x, h0.y, h1.x, h1.y));
                    xl = __builtin_bit_cast(bf16x8, make_uint4(l0.x, l0.y, l1.x, l1.y));
                }
#pragma unroll
                for (int n = 0; n < C::NB; ++n) { MFMA_T(acc[m][n], wh[n], wl[n], xh, xl); }
            }
        }
        if (chunk + 1 < C::NCHUNK) {
            __syncthreads();
            GEN_LAND();
        }
    }
#undef GEN_FETCH
#undef GEN_LAND
#undef F4

    load_bias<COUT, C::NB>(a, co0 + 4 * kg, bias);
    if constexpr (OUT_SP) {
        // ReLU(acc + bias) as split fp16 planes for conv3.hip's kernels: the lane's 8 channels {16(2j) + 4kg + r, 16(2j+1) + 4kg + r}
        static_assert(COUT == 64 && C::NB == 4 && !OUT_STATE, "plane output: the 64-channel intermediates only");
        unsigned char* const sp_img = a.out_sp + (size_t)b * a.out_sp_img_bytes;
#pragma unroll
        for (int m = 0; m < C::MR; ++m) {
            const int oy = ty0 + wave * C::MR + m, ox = tx0 + lrow;
            if (oy >= a.Hout || ox >= a.Wout) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float f8[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int n = 2 * j + (e >> 2);
                    const float bb = e & 2 ? (e & 1 ? bias[n].w : bias[n].z) : (e & 1 ? bias[n].y : bias[n].x);
                    const float v = acc[m][n][e & 3] + bb;
                    f8[e] = v > 0.f ? v : 0.f;
                }
                u32x4 hi, lo;
                split8_sp(f8, hi, lo, range_amax);
                *(u32x4*)(sp_img + sp_offset(j * 4 + kg, 0, oy, ox, a.Hout, a.Wout)) = hi;
                *(u32x4*)(sp_img + sp_offset(j * 4 + kg, 1, oy, ox, a.Hout, a.Wout)) = lo;
            }
        }
        vst_note_range(range_amax);
        return;
    }
    if constexpr (OUT_H16) {
        static_assert(!OUT_STATE && !OUT_SP, "fp16 output: the h1 intermediates only");
        _Float16* const o16 = (_Float16*)a.out + (size_t)b * a.out_img_stride;
#pragma unroll
        for (int m = 0; m < C::MR; ++m)
#pragma unroll
            for (int n = 0; n < C::NB; ++n) {
                const int oy = ty0 + wave * C::MR + m, ox = tx0 + lrow, co = co0 + 4 * kg + n * 16;
                if (oy >= a.Hout || ox >= a.Wout || co >= COUT) continue;
                const float r[4] = {acc[m][n][0] + bias[n].x, acc[m][n][1] + bias[n].y, acc[m][n][2] + bias[n].z, acc[m][n][3] + bias[n].w};
                typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
                f16x4 h;
                range_amax = fmaxf(fmaxf(range_amax, r[0]), fmaxf(fmaxf(r[1], r[2]), r[3]));
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = (_Float16)__builtin_amdgcn_fmed3f(r[e], 0.f, 65504.f);     // ReLU, saturating
                *(f16x4*)(o16 + ((size_t)oy * a.Wout + ox) * COUT + co) = h;
            }
        vst_note_range(range_amax);
        VST_TRACE_END_(2, CIN, COUT)
        return;
    }
    if constexpr (TERMS == 2) vst_note_range(range_amax);
    if (OUT_STATE && !EARLY_OLD) fetch_old();
    if (interior) store_tile<COUT, OUT_STATE, C::MR, C::NB, true>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, co0 + 4 * kg, acc, bias, old);
    else store_tile<COUT, OUT_STATE, C::MR, C::NB>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, co0 + 4 * kg, acc, bias, old);
    VST_TRACE_END_(2, CIN, COUT)
}

// ---- conv.4 + conv.7 of one stage-1 / stage-2 coupling block in one launch -----------------------------------------
// h2 = ReLU(conv.4(h1)) never goes to HBM: the workgroup computes it for its 16x16 tile plus a one-pixel ring
// (18x18 positions, from a 20x20 region of h1) into the LDS image that conv.7's MFMAs read, then does
// dst += sign * (conv.7(h2) + bias).  ReflectionPad of h2 (RevResNet.py:85): an in-image pixel one step inside the
// border also writes the mirrored ring slot.  LDS: [h2 image][ union { h1 region + conv.4 weights ; conv.7 weights } ].
template <int CIN, bool NO_LO = false>
__device__ __forceinline__ void read_x_small(const unsigned char* img_hi, const unsigned char* img_lo, int nslot,
                                             int slot00, int iw, int ks, int kg, bf16x8& xh, bf16x8& xl) {
    if (CIN == 16) {
        int tap = 2 * ks + (kg >> 1);
        tap = tap > 8 ? 8 : tap;
        const int slot = slot00 + (tap / 3) * iw + tap % 3;
        const int aoff = ((kg & 1) * nslot + slot) * 16;
        xh = __builtin_bit_cast(bf16x8, *(const uint4*)(img_hi + aoff));
        if (!NO_LO) xl = __builtin_bit_cast(bf16x8, *(const uint4*)(img_lo + aoff)); else xl = xh;
    } else {
        int t0 = 8 * ks + 2 * kg;
        t0 = t0 > 8 ? 8 : t0;
        const int t1 = t0 + 1 > 8 ? 8 : t0 + 1;
        const int s0 = slot00 + (t0 / 3) * iw + t0 % 3, s1 = slot00 + (t1 / 3) * iw + t1 % 3;
        const uint2 h0 = *(const uint2*)(img_hi + s0 * 8), h1 = *(const uint2*)(img_hi + s1 * 8);
        xh = __builtin_bit_cast(bf16x8, make_uint4(h0.x, h0.y, h1.x, h1.y));
        if (!NO_LO) {
            const uint2 l0 = *(const uint2*)(img_lo + s0 * 8), l1 = *(const uint2*)(img_lo + s1 * 8);
            xl = __builtin_bit_cast(bf16x8, make_uint4(l0.x, l0.y, l1.x, l1.y));
        } else {
            xl = xh;
        }
    }
}

template <int MID, int CH, int TERMS = 3, int MR = 4, bool H16 = false>
struct PairCfg {
    using C7 = ConvCfg<MID, CH, 1, MR>;
    // h1 region (TH + 4 rows x 20 columns), h2 ring region (TH + 2 rows x 18 columns) of a TH x 16 tile, TH = 4 MR
    static constexpr int R1 = 20, N1SLOT = (4 * MR + 4) * R1, RW = 18, RH = 4 * MR + 2, NPX = RH * RW, NBLK = (NPX + 15) / 16;
    static constexpr int H1_PLANE = MID == 4 ? N1SLOT * 8 : C7::CIG * N1SLOT * 16;
    static constexpr int W4_PLANE = C7::KS * 4 * 16 * 16;
    // MID == 16: conv.7's 40 KB of weights take over the h1 region + conv.4 weights once conv.4 is done (62 KB, two
    // workgroups per CU); MID == 4: everything is small, conv.7's weights get their own region (one barrier fewer)
    static constexpr bool ALIAS = MID == 16;
    static constexpr int WPL = TERMS == 3 ? 2 : 1;            // weight planes in LDS (hi + lo, or the fp16 plane alone)
    static constexpr int H1W4 = (H16 ? 1 : 2) * H1_PLANE + WPL * W4_PLANE;   // H16: h1 arrives as fp16, one plane
    static constexpr int U_BYTES = ALIAS ? (H1W4 > WPL * C7::B_PLANE ? H1W4 : WPL * C7::B_PLANE) : H1W4 + WPL * C7::B_PLANE;
    static constexpr int LDS_BYTES = 2 * C7::A_PLANE + U_BYTES;
};

// H16: h1 is fp16 in HBM (conv_mfma_kernel<..., OUT_H16>): it is copied into the LDS image as it is and conv.4 issues one
// MFMA per product
// OUT_RGB (block 0 of an inverse pass, the last one): injective_pad.inverse keeps channels 0..C-1 of x1 = y1 - F(x2)
// (RevResNet.py:233-235), so the lanes that hold them write old - (acc + bias) straight into the NCHW image (or, for the uint8
// edge, mul(255).clamp.byte() HWC like unpack_output_u8_kernel) and nothing goes back to the state: the same MFMAs and the same
// final subtraction as the state form followed by the unpack kernel, without the state write, the unpack's read and its launch.
template <int MID, int CH, int TERMS = 3, int MR = 4, bool H16 = false, bool OUT_RGB = false>
__global__ __launch_bounds__(256, (MID == 16 && TERMS == 2) ? 3 : 1) void conv_pair_kernel(const ConvArgs a) {
    static_assert(!H16 || TERMS == 2, "fp16 h1: the 2-term kernels only");
    static_assert(!OUT_RGB || (MID == 4 && CH == 16), "image output: the 16-channel blocks only");
    using P = PairCfg<MID, CH, TERMS, MR, H16>;
    using C = typename P::C7;
    static_assert(C::NCHUNK == 1 && C::NCOT == 1, "single-chunk shapes");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const a_hi = smem;                        // h2 image (conv.7's activation image)
    unsigned char* const a_lo = smem + C::A_PLANE;
    unsigned char* const u0 = smem + 2 * C::A_PLANE;
    unsigned char* const b_hi = P::ALIAS ? u0 : u0 + P::H1W4;   // conv.7 weights (aliased: valid after conv.4 is done)
    unsigned char* const b_lo = TERMS == 3 ? b_hi + C::B_PLANE : b_hi;
    unsigned char* const h1_hi = u0;                         // h1 region + conv.4 weights (before)
    unsigned char* const h1_lo = H16 ? u0 : u0 + P::H1_PLANE;           // (H16: no lo plane)
    unsigned char* const w4s_hi = u0 + (H16 ? 1 : 2) * P::H1_PLANE;
    unsigned char* const w4s_lo = TERMS == 3 ? w4s_hi + P::W4_PLANE : w4s_hi;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 15, kg = lane >> 4;
    int bx, by, b;
    if (!xcd_tile(a, bx, by, b)) return;
    float range_amax = 0.f;
    VST_TRACE_BEGIN(1)
    const int tx0 = bx * C::TW, ty0 = by * C::TH;
    const int H = a.Hout, W = a.Wout;                        // h1, h2 and the output view share one resolution
    const float* const in_img = a.in + (size_t)b * a.in_img_stride;
    float* const out_img = a.out + (size_t)b * a.out_img_stride;
    const PackedConvLayout PL7 = packed_conv_layout(CH, MID), PL4 = packed_conv_layout(MID, MID);
    const unsigned char* const w7_hi = a.packed + (TERMS == 3 ? PL7.f32_bytes : PL7.f16_offset);
    const unsigned char* const w7_lo = w7_hi + PL7.frag_bytes;              // (the lo planes are not read when TERMS == 2)
    const unsigned char* const w4_hi = a.packed1 + (TERMS == 3 ? PL4.f32_bytes : PL4.f16_offset);
    const unsigned char* const w4_lo = w4_hi + PL4.frag_bytes;

    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    constexpr int H1_ITEMS = MID == 4 ? P::N1SLOT : P::N1SLOT * C::CIG, H1IT = (H1_ITEMS + 255) / 256, NV = MID == 4 ? 1 : 2;
    constexpr int W4_ITEMS = C::KS * 4 * 16, W4IT = (W4_ITEMS + 255) / 256;
    constexpr int W7_ITEMS = C::KS * 4 * C::NT, W7IT = (W7_ITEMS + 255) / 256;
    f32x4 hreg[H1IT][NV];
    u32x4 h16reg[H16 ? H1IT : 1];                            // (H16: raw fp16 words - never routed through float registers)
    u32x4 w4reg[W4IT][2], w7reg[W7IT][2];
    // ---- fetch everything this workgroup reads, back to back ---------------------------------------------------------
#pragma unroll
    for (int it = 0; it < W4IT; ++it) {
        int idx = it * 256 + tid;
        idx = idx < W4_ITEMS ? idx : W4_ITEMS - 1;
        w4reg[it][0] = *(const u32x4*)(w4_hi + (size_t)idx * 16);      // coutp == 16: fragment order is already [r][co]
        if (TERMS == 3) w4reg[it][1] = *(const u32x4*)(w4_lo + (size_t)idx * 16);
    }
#pragma unroll
    for (int it = 0; it < H1IT; ++it) {
        int idx = it * 256 + tid;
        idx = idx < H1_ITEMS ? idx : H1_ITEMS - 1;
        const int cig = MID == 4 ? 0 : idx % C::CIG, slot = MID == 4 ? idx : idx / C::CIG;
        const int iy = slot / P::R1, ix = slot - iy * P::R1;
        const int gy = reflect_clamp(ty0 - 2 + iy, H), gx = reflect_clamp(tx0 - 2 + ix, W);
        if constexpr (H16) {                                   // 8 (MID == 16) or 4 (MID == 4) fp16 values: the operand itself
            const _Float16* p16 = (const _Float16*)a.in + (size_t)b * a.in_img_stride + ((size_t)gy * W + gx) * MID + cig * 8;
            if (MID == 4) { const uint2 v = *(const uint2*)p16; h16reg[it] = u32x4{v.x, v.y, 0u, 0u}; }
            else h16reg[it] = *(const u32x4*)p16;
        } else {
            const float* p = in_img + ((size_t)gy * W + gx) * MID + cig * 8;
            hreg[it][0] = *(const f32x4*)p;
            if (NV == 2) hreg[it][NV - 1] = *(const f32x4*)(p + 4);
        }
    }
#pragma unroll
    for (int it = 0; it < W7IT; ++it) {
        int idx = it * 256 + tid;
        idx = idx < W7_ITEMS ? idx : W7_ITEMS - 1;
        const int co = idx % C::NT, r = idx / C::NT;
        const size_t src = ((size_t)r * C::COUTP + co) * 16;
        w7reg[it][0] = *(const u32x4*)(w7_hi + src);
        if (TERMS == 3) w7reg[it][1] = *(const u32x4*)(w7_lo + src);
    }
    float4 bias[C::NB], old[C::MR][C::NB];
    const bool interior = ty0 + C::TH <= H && tx0 + C::TW <= W;
    constexpr bool EARLY_OLD = C::MR * C::NB >= 16 && TERMS == 3 && !OUT_RGB;   // (2-term form: three workgroups per CU need <= 168 VGPRs)
#define PAIR_FETCH_OLD()                                                                                         \
    if (interior) load_old<CH, C::MR, C::NB, true>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, 4 * kg, old);   \
    else load_old<CH, C::MR, C::NB>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, 4 * kg, old);
    if (EARLY_OLD) { PAIR_FETCH_OLD(); }

    // ---- land h1 (bf16 split) and conv.4's weights --------------------------------------------------------------------
#define F4(v_) make_float4((v_)[0], (v_)[1], (v_)[2], (v_)[3])
#pragma unroll
    for (int it = 0; it < H1IT; ++it) {
        int idx = it * 256 + tid;
        idx = idx < H1_ITEMS ? idx : H1_ITEMS - 1;
        if constexpr (H16) {
            if (MID == 4) {
                *(uint2*)(h1_hi + idx * 8) = make_uint2(h16reg[it][0], h16reg[it][1]);
            } else {
                const int cig = idx % C::CIG, slot = idx / C::CIG;
                *(u32x4*)(h1_hi + (cig * P::N1SLOT + slot) * 16) = h16reg[it];
            }
        } else if (MID == 4) {
            uint2 h, l;
            SPLIT4_T(F4(hreg[it][0]), h, l);
            *(uint2*)(h1_hi + idx * 8) = h;
            *(uint2*)(h1_lo + idx * 8) = l;
        } else {
            const int cig = idx % C::CIG, slot = idx / C::CIG;
            uint4 h, l;
            SPLIT8_T(F4(hreg[it][0]), F4(hreg[it][NV - 1]), h, l);
            *(uint4*)(h1_hi + (cig * P::N1SLOT + slot) * 16) = h;
            *(uint4*)(h1_lo + (cig * P::N1SLOT + slot) * 16) = l;
        }
    }
#undef F4
#pragma unroll
    for (int it = 0; it < W4IT; ++it) {
        int idx = it * 256 + tid;
        idx = idx < W4_ITEMS ? idx : W4_ITEMS - 1;
        *(u32x4*)(w4s_hi + idx * 16) = w4reg[it][0];
        if (TERMS == 3) *(u32x4*)(w4s_lo + idx * 16) = w4reg[it][1];
    }
#define LAND_W7()                                                                                  \
    _Pragma("unroll") for (int it = 0; it < W7IT; ++it) {                                          \
        int idx = it * 256 + tid;                                                                  \
        idx = idx < W7_ITEMS ? idx : W7_ITEMS - 1;                                                 \
        *(u32x4*)(b_hi + idx * 16) = w7reg[it][0];                                                 \
        if (TERMS == 3) *(u32x4*)(b_lo + idx * 16) = w7reg[it][1];                                 \
    }
    if (!P::ALIAS) { LAND_W7(); }
    __syncthreads();

    // ---- conv.4 on the 18x18 ring region: 16-pixel blocks of the linearised region, one 16-channel block ---------------
    {
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * kg < MID) b4 = *(const float4*)(a.bias1 + 4 * kg);
        const bool ring_inside = ty0 >= 1 && tx0 >= 1 && ty0 + C::TH + 1 <= H && tx0 + 17 <= W;
        constexpr bool HOIST = MID == 4;                        // conv.4's fragments are the same for every pixel block;
        bf16x8 w4h[HOIST ? C::KS : 1], w4l[HOIST ? C::KS : 1];   // keep them in registers where there is room
        if (HOIST) {
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks) {
                const int boff = ((ks * 4 + kg) * 16 + lrow) * 16;
                w4h[HOIST ? ks : 0] = __builtin_bit_cast(bf16x8, *(const uint4*)(w4s_hi + boff));
                w4l[HOIST ? ks : 0] = __builtin_bit_cast(bf16x8, *(const uint4*)(w4s_lo + boff));
            }
        }
        // two pixel blocks per iteration (independent MFMA chains); the second may be past the end (clamped, not written)
        for (int blk0 = wave; blk0 < P::NBLK; blk0 += 8) {
            f32x4 acc4[2];
            int ryv[2], rxv[2];
            bool okv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int p = (blk0 + 4 * u) * 16 + lrow;
                okv[u] = p < P::NPX;
                p = okv[u] ? p : P::NPX - 1;
                ryv[u] = p / P::RW; rxv[u] = p - ryv[u] * P::RW;
                acc4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks) {
                bf16x8 wh, wl;
                if (HOIST) {
                    wh = w4h[HOIST ? ks : 0]; wl = w4l[HOIST ? ks : 0];
                } else {
                    const int boff = ((ks * 4 + kg) * 16 + lrow) * 16;
                    wh = __builtin_bit_cast(bf16x8, *(const uint4*)(w4s_hi + boff));
                    wl = __builtin_bit_cast(bf16x8, *(const uint4*)(w4s_lo + boff));
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    bf16x8 xh, xl;
                    read_x_small<MID, H16>(h1_hi, h1_lo, P::N1SLOT, ryv[u] * P::R1 + rxv[u], P::R1, ks, kg, xh, xl);
                    if constexpr (H16) {
                        acc4[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xh), acc4[u], 0, 0, 0);
                    } else {
                        MFMA_T(acc4[u], wh, wl, xh, xl);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                // lane (lrow, kg) holds channels 4kg..4kg+3 of region pixel (ry, rx)
                const int ry = ryv[u], rx = rxv[u];
                float4 v = make_float4(acc4[u][0] + b4.x, acc4[u][1] + b4.y, acc4[u][2] + b4.z, acc4[u][3] + b4.w);
                v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f;
                v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
                uint2 h, l;
                SPLIT4_T(v, h, l);
#define PAIR_PUT(slot_)                                                                            \
                if (MID == 4) {                                                                    \
                    *(uint2*)(a_hi + (slot_) * 8) = h;                                             \
                    *(uint2*)(a_lo + (slot_) * 8) = l;                                             \
                } else {                                                                           \
                    const int off_ = ((kg >> 1) * C::NSLOT + (slot_)) * 16 + (kg & 1) * 8;         \
                    *(uint2*)(a_hi + off_) = h;                                                    \
                    *(uint2*)(a_lo + off_) = l;                                                    \
                }
                if (ring_inside) {                           // uniform: the whole 18x18 ring region lies inside the image
                    if (okv[u] && 4 * kg < MID) { PAIR_PUT(ry * C::IW + rx); }
                } else {
                    const int gy = ty0 - 1 + ry, gx = tx0 - 1 + rx;
                    if (okv[u] && 4 * kg < MID && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                        // own slot + the mirrored ring slots (ReflectionPad2d(1) of h2): row -1 <- row 1, row H <- row H-2,
                        // same in x; where no mirror applies the same slot is written again
                        const int my = gy == 1 ? -2 : (gy == H - 2 ? 2 : 0), mx = gx == 1 ? -2 : (gx == W - 2 ? 2 : 0);
                        int sy = ry + my, sx = rx + mx;
                        sy = (sy < 0 || sy >= P::RH) ? ry : sy;
                        sx = (sx < 0 || sx >= P::RW) ? rx : sx;
                        PAIR_PUT(ry * C::IW + rx);
                        PAIR_PUT(sy * C::IW + rx);
                        PAIR_PUT(ry * C::IW + sx);
                        PAIR_PUT(sy * C::IW + sx);
                    }
                }
#undef PAIR_PUT
            }
        }
    }
    __syncthreads();                                         // h2 image complete; h1 region and conv.4 weights are dead
    if (P::ALIAS) {
        LAND_W7();
        __syncthreads();
    }
#undef LAND_W7

    // ---- conv.7 from the LDS image, state read-modify-write -------------------------------------------------------------
    f32x4 acc[C::MR][C::NB];
#pragma unroll
    for (int m = 0; m < C::MR; ++m)
#pragma unroll
        for (int n = 0; n < C::NB; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int slot_base = (wave * C::MR) * C::IW + lrow;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
        bf16x8 wh[C::NB], wl[C::NB];
#pragma unroll
        for (int n = 0; n < C::NB; ++n) {
            const int boff = ((ks * 4 + kg) * C::NT + n * 16 + lrow) * 16;
            wh[n] = __builtin_bit_cast(bf16x8, *(const uint4*)(b_hi + boff));
            wl[n] = __builtin_bit_cast(bf16x8, *(const uint4*)(b_lo + boff));
        }
#pragma unroll
        for (int m = 0; m < C::MR; ++m) {
            bf16x8 xh, xl;
            read_x_small<MID>(a_hi, a_lo, C::NSLOT, slot_base + m * C::IW, C::IW, ks, kg, xh, xl);
#pragma unroll
            for (int n = 0; n < C::NB; ++n) { MFMA_T(acc[m][n], wh[n], wl[n], xh, xl); }
        }
    }
    load_bias<CH, C::NB>(a, 4 * kg, bias);
    if constexpr (TERMS == 2) vst_note_range(range_amax);
    if constexpr (OUT_RGB) {
        // lane (lrow, kg) holds channels 4 kg .. 4 kg + 3 of pixel (oy, tx0 + lrow): a plane store per kept channel, coalesced over
        // the 16 pixels of the block
        const int ox = tx0 + lrow, nc = a.rgb_u8 ? 3 : a.rgb_c;
        const size_t plane = (size_t)H * W;
#pragma unroll
        for (int m = 0; m < C::MR; ++m) {
            const int oy = ty0 + wave * C::MR + m;
            if (oy >= H || ox >= W || 4 * kg >= nc) continue;
            const float4 o = *(const float4*)(out_img + zc_offset(0, oy, ox, a.Wq) + 4 * kg);
            float4 r = make_float4(acc[m][0][0] + bias[0].x, acc[m][0][1] + bias[0].y, acc[m][0][2] + bias[0].z,
                                   acc[m][0][3] + bias[0].w);
            r = make_float4(o.x + a.sign * r.x, o.y + a.sign * r.y, o.z + a.sign * r.z, o.w + a.sign * r.w);
            const float c[4] = {r.x, r.y, r.z, r.w};
            if (a.rgb_u8) {
                unsigned char* dst = a.rgb_u8 + ((size_t)b * plane + (size_t)oy * W + ox) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float t = c[k] * 255.f;
                    t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);       // (NaN falls through both compares; byte() of it is 0)
                    dst[k] = (unsigned char)t;                         // truncation toward zero
                }
            } else {
                float* dst = a.rgb + ((size_t)b * a.rgb_c + 4 * kg) * plane + (size_t)oy * W + ox;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * kg + k < nc) dst[k * plane] = c[k];
            }
        }
        VST_TRACE_END_(1, MID, CH)
        return;
    }
    if (!EARLY_OLD) { PAIR_FETCH_OLD(); }
#undef PAIR_FETCH_OLD
    if (interior) store_tile<CH, true, C::MR, C::NB, true>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, 4 * kg, acc, bias, old);
    else store_tile<CH, true, C::MR, C::NB>(a, out_img, ty0 + wave * C::MR, tx0 + lrow, 4 * kg, acc, bias, old);
    VST_TRACE_END_(1, MID, CH)
}

// ---- pipelined kernel for the MFMA-bound shapes: CIN in {64,256}, COUT in {64,256}, stride 1 --------
// A stage = (32-channel chunk, tap row dy) = 3 k-steps = 144 MFMAs per wave.  Two activation buffers
// and two weight buffers in LDS; while stage s computes, the wave prefetches stage s+1's weights and a
// third of the next chunk's activations into registers and writes them to the other buffers after its
// MFMAs (one barrier per stage).  With COUT = 256 the four 64-channel output tiles are looped inside
// the workgroup: the activation image (both chunks) stays resident, only weights stream.
template <int CIN, int COUT, int NW_ = 8, int MR_ = 2>
struct PipeCfg {
    // NW_ = 8, MR_ = 2: two waves per SIMD on a 16 x 16 tile, the workgroup owns its CU (135 KB of LDS).
    // NW_ = 4, MR_ = 2 (the "lean" form): one wave per SIMD on an 8 x 16 tile, 96 KB of LDS and <= 256 VGPRs, so that an HBM-bound
    // stage-1 / stage-2 workgroup of ANOTHER frame's stream (<= 61 KB, <= 256 VGPRs) shares the CU.  (Two lean workgroups do not:
    // 2 x 96 KB is more than the CU's 160 KB.)
    // NW_ = 4, MR_ = 4 (the "wide" form): one wave per SIMD on the 16 x 16 tile of the 8-wave form (same LDS images, 135 KB), each
    // wave a 64 co x 64 px register tile: 16 fragment reads per 48 MFMAs instead of 12 per 24, and the whole 512-register file
    static constexpr int NW = NW_, NTHR = 64 * NW, MR = MR_;  // each wave owns MR tile rows (NTHR == launch bounds)
    static constexpr int NT = 64, NB = 4, TH = MR * NW, IW = 18, NPIX = (TH + 2) * IW, NSLOT = (NPIX + 15) / 16 * 16;
    static constexpr int NCHUNK = CIN / 32, NCOT = COUT / 64;
    static constexpr int A_PLANE = 4 * NSLOT * 16, A_BUF = 2 * A_PLANE;       // 43008 / 24576 (hi + lo planes of one 32-channel chunk)
    static constexpr int B_PLANE = 3 * 4 * 64 * 16, B_BUF = 2 * B_PLANE;      // 24576 (hi + lo, 3 k-steps x 64 channels)
    static constexpr int LDS_BYTES = 2 * A_BUF + 2 * B_BUF;                   // 135168 / 98304
    static constexpr int A_PART = NPIX * 4 / 3;                               // 432 / 240 (slot, cig) items per stage
    static constexpr int A_ITEMS = ((A_PART / 4 + 15) / 16 * 64 + NTHR - 1) / NTHR;   // per thread and part (lanes in 16-slot x 4-plane groups)
    static constexpr int B_ITEMS = 2 * 768 / NTHR;                            // uint4 per thread and stage
    static_assert(NPIX % 3 == 0, "three equal parts");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// Pipeline: a stage = (32-channel chunk, tap row dy) = 3 k-steps.  Two activation buffers and two weight
// buffers in LDS.  While stage s computes, the wave issues the global loads of stage s+2's weights and of a
// third of the next chunk's activations into registers (two register sets indexed by the compile-time
// stage parity: six stages are unrolled per loop body) and writes what it loaded during stage s-1 into the
// buffers of stage s+1; one barrier per stage.  Fragments are double-buffered in registers across k-steps.
// With COUT = 256 the four 64-channel output slices are looped inside the workgroup: the activation image
// (both chunks) stays resident, only weights stream.
// wide form of conv_pipe_kernel: the order in which one k-step's instructions issue (LLVM SchedGroupMask: MFMA 0x8, VMEM read 0x20,
// DS read 0x100, DS write 0x200).  Every MFMA is followed by the fillers of its gap: a fragment read in each of the first 2 * NDSR
// even gaps, a global load (NVM) or an LDS store (NDW) in the odd ones.  Other instructions (VALU) are placed by the scheduler.
template <int NDSR, int NVM, int NDW>
__device__ __forceinline__ void wide_interleave() {
#pragma unroll
    for (int i = 0; i < 48; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (i % 2 == 0 && i / 2 < NDSR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        if (i % 2 == 1 && i / 2 < NVM) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        if (i % 2 == 1 && i / 2 < NDW) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
}

// The wide form (NW = 4, MR = 4) issues the same instructions per accumulator but places them differently: a stage's staging
// (global loads, bf16 split, LDS stores) and the next k-step's fragment reads go BETWEEN its MFMAs (sched_group_barrier), in the
// issue shadow of the lone wave's matrix stream, instead of in clusters in front of them.
template <int CIN, int COUT, bool IN_STATE, bool OUT_STATE, int NW = 8, int MR = 2>
__global__ __launch_bounds__(64 * NW, (NW == 4 && MR == 2) ? 2 : 1) void conv_pipe_kernel(const ConvArgs a) {
    using C = PipeCfg<CIN, COUT, NW, MR>;
    constexpr bool WIDE = NW == 4 && MR == 4;
    constexpr bool PEEL = WIDE && COUT == 64;                // the wide kernels with ONE output slice: see the prologue and the loop
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const Abuf = smem;
    unsigned char* const Bbuf = smem + 2 * C::A_BUF;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 15, kg = lane >> 4;
    int bx, by, b;
    if (!xcd_tile(a, bx, by, b)) return;
    VST_TRACE_BEGIN(4)
    const int tx0 = bx * 16, ty0 = by * C::TH;
    const float* const in_img = a.in + (size_t)b * a.in_img_stride;
    float* const out_img = a.out + (size_t)b * a.out_img_stride;
    const PackedConvLayout PL = packed_conv_layout(COUT, CIN);
    const unsigned char* const w_plane0 = a.packed + PL.f32_bytes;

    // activation staging: each third ("part") of the 18x18 x (4 channel-groups) image is 432 (slot, cig)
    // items, A_ITEMS per thread.  All uses index these arrays with compile-time constants (the tap-row
    // stages are unrolled), so they stay in registers.  Threads past the end repeat the last item.
    unsigned a_src[3][C::A_ITEMS], a_dst[3][C::A_ITEMS];
#define A_TABLE(part)                                                                   \
    _Pragma("unroll") for (int it = 0; it < C::A_ITEMS; ++it) {                         \
        /* 16 consecutive lanes take 16 consecutive slots of ONE channel-group plane (conflict-free ds_write_b128; */ \
        /* cig-fastest would put 4 lanes on the same banks) and together still read whole 128-byte pixel chunks */    \
        const int j = it * C::NTHR + tid;                                               \
        int sl = (j >> 6) * 16 + (j & 15);                       /* slot within this part (108 slots per part) */     \
        sl = sl < C::A_PART / 4 ? sl : C::A_PART / 4 - 1;                               \
        const int cig = (j >> 4) & 3, slot = (part) * (C::A_PART / 4) + sl;             \
        const int iy = slot / C::IW, ix = slot - iy * C::IW;                            \
        const int gy = reflect_clamp(ty0 - 1 + iy, a.Hin), gx = reflect_clamp(tx0 - 1 + ix, a.Win); \
        const size_t off = IN_STATE ? zc_offset(vst_level_of_channels(CIN), gy, gx, a.Wq) \
                                    : ((size_t)gy * a.Win + gx) * CIN;                  \
        a_src[part][it] = (unsigned)(off + cig * 8);                                    \
        a_dst[part][it] = (cig * C::NSLOT + slot) * 16;                                 \
    }
    // (the one-slice wide kernels fill the tables of a part right before that part's loads, under the latency of the loads
    // before them; in the 64 -> 256 kernel that order was not shown to pay)
    if constexpr (!PEEL) {
#pragma unroll
        for (int part = 0; part < 3; ++part) { A_TABLE(part); }
    }
    // (native vector arrays filled by macros, every index a compile-time constant after unrolling: as structs returned from
    // lambdas the six-item stage of the 4-wave form was demoted to scratch)
    typedef f32x4 APart[C::A_ITEMS][2];
    typedef u32x4 BStage[C::B_ITEMS];
#define LOAD_A(r, chunk, part)                                                          \
    _Pragma("unroll") for (int it_ = 0; it_ < C::A_ITEMS; ++it_) {                      \
        const float* p_ = in_img + a_src[part][it_] + (chunk) * 32;                     \
        r[it_][0] = *(const f32x4*)p_; r[it_][1] = *(const f32x4*)(p_ + 4);             \
    }
#define F4_(v_) make_float4((v_)[0], (v_)[1], (v_)[2], (v_)[3])
#define STORE_A(buf, part, r)                                                           \
    _Pragma("unroll") for (int it_ = 0; it_ < C::A_ITEMS; ++it_) {                      \
        unsigned char* base_ = Abuf + (buf) * C::A_BUF;                                 \
        uint4 h_, l_;                                                                   \
        split8(F4_(r[it_][0]), F4_(r[it_][1]), h_, l_);                                 \
        *(uint4*)(base_ + a_dst[part][it_]) = h_;                                       \
        *(uint4*)(base_ + C::A_PLANE + a_dst[part][it_]) = l_;                          \
    }
    // weights of stage (q = cot*NCHUNK + chunk, dy): 2 planes (hi, lo) x 3 k-steps x 256 uint4 = 1536 items
    int b_off[C::B_ITEMS], b_dst[C::B_ITEMS];
#pragma unroll
    for (int it = 0; it < C::B_ITEMS; ++it) {
        if constexpr (NW == 4) {      // item it = (plane it / 3, k-step it % 3, thread = (kgi, co)): one base + constants
            const int plane = it / 3, k3 = it % 3, kgi = tid >> 6, co = tid & 63;
            b_off[it] = ((kgi * COUT + co) * 16) + (int)(plane * PL.frag_bytes) + k3 * 4 * COUT * 16;
            b_dst[it] = tid * 16 + plane * C::B_PLANE + k3 * 256 * 16;
        } else {
            const int idx = it * C::NTHR + tid;
            const int plane = idx >= 768, r = idx - plane * 768;
            const int k3 = r >> 8, kgi = (r >> 6) & 3, co = r & 63;
            b_off[it] = (int)(plane * PL.frag_bytes) + ((k3 * 4 + kgi) * COUT + co) * 16;
            b_dst[it] = plane * C::B_PLANE + r * 16;
        }
    }
#define LOAD_B(r, q_, dy_)                                                              \
    {                                                                                   \
        const int cot_ = (q_) / C::NCHUNK, chunk_ = (q_) - cot_ * C::NCHUNK;            \
        const unsigned char* src_ = w_plane0 + ((size_t)(chunk_ * 9 + (dy_) * 3) * 4 * COUT + cot_ * 64) * 16;   \
        _Pragma("unroll") for (int it_ = 0; it_ < C::B_ITEMS; ++it_) r[it_] = *(const u32x4*)(src_ + b_off[it_]); \
    }
#define STORE_B(buf, r)                                                                 \
    { _Pragma("unroll") for (int it_ = 0; it_ < C::B_ITEMS; ++it_) *(u32x4*)(Bbuf + (buf) * C::B_BUF + b_dst[it_]) = r[it_]; }
    struct Frags { bf16x8 wh[4], wl[4], xh[C::MR], xl[C::MR]; };
    auto read_frags = [&](Frags& f, const unsigned char* Ab, const unsigned char* Bb, int k3) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            f.wh[n] = __builtin_bit_cast(bf16x8, *(const uint4*)(Bb + (k3 * 256 + n * 16) * 16));
            f.wl[n] = __builtin_bit_cast(bf16x8, *(const uint4*)(Bb + C::B_PLANE + (k3 * 256 + n * 16) * 16));
        }
#pragma unroll
        for (int m = 0; m < C::MR; ++m) {
            f.xh[m] = __builtin_bit_cast(bf16x8, *(const uint4*)(Ab + (m * C::IW + k3) * 16));
            f.xl[m] = __builtin_bit_cast(bf16x8, *(const uint4*)(Ab + C::A_PLANE + (m * C::IW + k3) * 16));
        }
    };

    constexpr int Q = C::NCOT * C::NCHUNK;                  // (output slice, chunk) pairs; stage s = 3q + dy
    static_assert(Q % 2 == 0, "stage parity is static only for an even number of (slice, chunk) pairs");
    // ---- prologue: chunk 0 activations + stage 0 weights land in LDS; stage 1 weights and the first third of
    //      chunk 1 stay in registers (they are written to LDS during stage 0).  Register set[s&1] is loaded during
    //      stage s and stored during stage s+1.
    // (the lean form stages twice as much per thread: it keeps ONE register set - a stage lands what the previous stage
    // loaded and then reuses the registers for its own loads; the 8-wave form issues its loads first, into a second set)
    constexpr bool ONE_SET = NW == 4 && !WIDE;
#define RS(i_) (ONE_SET ? 0 : (i_))
    BStage rb[ONE_SET ? 1 : 2];
    APart ra[ONE_SET ? 1 : 2];
    if constexpr (PEEL) {
        // the lone wave of a SIMD has nothing to overlap its address arithmetic with: every load goes out as soon as its own
        // addresses exist (the sched_barriers keep the scheduler from gathering the arithmetic in front of the first load), and
        // what arrives is landed in the order of issue (vmcnt counts in order)
        BStage rb0;
        LOAD_B(rb0, 0, 0);
        APart r0, r1, r2;
        A_TABLE(0); LOAD_A(r0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        A_TABLE(1); LOAD_A(r1, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        A_TABLE(2); LOAD_A(r2, 0, 2);
        __builtin_amdgcn_sched_barrier(0);
        LOAD_B(rb[1], 0, 1);
        if (C::NCHUNK > 1) LOAD_A(ra[1], 1, 0);
        STORE_B(0, rb0);
        STORE_A(0, 0, r0); STORE_A(0, 1, r1); STORE_A(0, 2, r2);
    } else {
        BStage rb0;
        LOAD_B(rb0, 0, 0);
        APart r0, r1, r2;
        LOAD_A(r0, 0, 0); LOAD_A(r1, 0, 1); LOAD_A(r2, 0, 2);
        LOAD_B(rb[RS(1)], 0, 1);
        if (C::NCHUNK > 1) LOAD_A(ra[RS(1)], 1, 0);
        STORE_A(0, 0, r0); STORE_A(0, 1, r1); STORE_A(0, 2, r2);
        STORE_B(0, rb0);
    }
    __syncthreads();

    f32x4 acc[C::MR][4];
#pragma unroll
    for (int m = 0; m < C::MR; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int slot_base = (wave * C::MR) * C::IW + lrow;
    const int oy0 = ty0 + wave * C::MR;
    float4 bias[4], old[C::MR][4];
    const bool full_tile = ty0 + C::TH <= a.Hout && tx0 + 16 <= a.Wout; // uniform: interior tiles skip all predicates
    // Kernels that loop several 64-channel output slices (the 64 -> 256 conv: four) DEFER a slice's stores: at the slice's end
    // the results are formed in place in `old` (old + sign * (acc + bias)), and the eight float4 stores per lane go out one per
    // k-step during the next slice's first chunk, between its MFMAs - all eight waves used to issue them together behind the
    // slice's last MFMA, in front of the stage barrier (a timing-only build without three of the four epilogues:
    // 59.5 -> 49.5 us).  `old` is free for that long: the next slice loads its own old values at its last stage.
    constexpr bool DEFER = OUT_STATE && C::NCOT > 1 && C::NCHUNK == 2;
    bool pending = false;                                    // uniform: `old` holds a finished slice whose stores are still due
    int pend_cot = 0;
    // unit u = (m, n) of the first chunk of a slice (MR * 4 units: the lean and 8-wave forms one per k-step, the wide form two)
#define DEFER_UNIT(unit_)                                                                                                             \
    {                                                                                                                                 \
        const int m_ = (unit_) >> 2, n_ = (unit_) & 3;                                                                                \
        if (pending) {                                         /* ... of the previous slice: its deferred store */                    \
            float4* p_ = full_tile ? out_ptr<COUT, OUT_STATE, true>(a, out_img, oy0 + m_, tx0 + lrow, pend_cot * 64 + 4 * kg + n_ * 16) \
                                   : out_ptr<COUT, OUT_STATE, false>(a, out_img, oy0 + m_, tx0 + lrow, pend_cot * 64 + 4 * kg + n_ * 16); \
            if (full_tile || p_) *p_ = old[m_][n_];                                                                                   \
        }                                                                                                                             \
        {                                                      /* ... of this slice: its old state value, see below */                \
            const float4* q_ = full_tile ? out_ptr<COUT, OUT_STATE, true>(a, out_img, oy0 + m_, tx0 + lrow, cot * 64 + 4 * kg + n_ * 16) \
                                         : out_ptr<COUT, OUT_STATE, false>(a, out_img, oy0 + m_, tx0 + lrow, cot * 64 + 4 * kg + n_ * 16); \
            old[m_][n_] = (full_tile || q_) ? *q_ : make_float4(0.f, 0.f, 0.f, 0.f);                                                  \
        }                                                                                                                             \
    }

    // The one-slice wide kernels (PEEL) run the loop over pairs of chunks in two passes: pass 0 the iterations before the last,
    // pass 1 (`tail`) the last one as a peeled copy in which q0 = Q - 2 is a constant.  After unrolling, every stage of the tail
    // knows whether anything is left to stage, so the stages near the end issue no loads and no LDS stores at all, and the
    // body of the other iterations stays branch-free and holds no output code.  With Q == 2 the tail is the whole loop.  All
    // other kernels make one pass over [0, Q).
    // (Like the stage parity `cur` below, this relies on the unrolled loops folding to constants; a generic lambda with the
    // tail as a template argument was built instead and changed the code of all nine kernels, one of them into scratch.)
    constexpr int NPASS = PEEL ? 2 : 1;
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
    const bool tail = PEEL && pass == 1;
    const int q0_begin = tail ? Q - 2 : 0, q0_end = (PEEL && !tail) ? Q - 2 : Q;
#pragma unroll 1
    for (int q0v = q0_begin; q0v < q0_end; q0v += 2) {
      const int q0 = tail ? Q - 2 : q0v;
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const int q = q0 + qq;
        const int cot = q / C::NCHUNK, chunk = q - cot * C::NCHUNK;
        const bool last_chunk = (!PEEL || tail) && chunk == C::NCHUNK - 1;      // (PEEL: the last chunk is in the tail)
        const bool first_chunk = PEEL ? tail && qq == 0 : chunk == 0;           // (... where the bias is fetched, too)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int s = q * 3 + dy;
            const int cur = (qq * 3 + dy) & 1;            // compile-time parity of s
            if constexpr (WIDE) {
                // ---- the wide form: the same loads, stores and MFMAs per stage as below, but the staging and the fragment reads
                //      are placed between the MFMAs of the stage's k-steps.  Loads still run two stages ahead and land one stage
                //      ahead (two register sets); the branches of the stage sit at its top and at the top of each k-step.
                //      NCOT == 1 kernels stage activations in every stage that has some left (A_ALWAYS; known at compile time, see
                //      PEEL); the 64 -> 256 kernel loads clamped weights in its last two stages, into a buffer nobody reads.
                constexpr bool A_ALWAYS = C::NCOT == 1;
                const int q2 = dy == 0 ? q : q + 1, dy2 = (dy + 2) % 3;      // weights of stage s+2
                const int qn = dy == 2 ? q + 1 : q, dyn = (dy + 1) % 3;      // activations landed during stage s+1
                const bool ld_b = !tail || q2 < Q, st_b = !tail || s + 1 < 3 * Q;            // (all true outside the tail)
                const bool ld_a = A_ALWAYS && (!tail || qn + 1 < C::NCHUNK), st_a = A_ALWAYS && (!tail || q + 1 < C::NCHUNK);
                if (DEFER ? (dy == 2 && last_chunk) : (dy == 0 && first_chunk)) load_bias<COUT, 4>(a, cot * 64 + 4 * kg, bias);
                if (!A_ALWAYS && q < C::NCHUNK - 1) STORE_A((chunk + 1) & 1, dy, ra[cur ^ 1]);
                if (!A_ALWAYS && qn < C::NCHUNK - 1) LOAD_A(ra[cur], qn + 1, dyn);
                if (OUT_STATE && !DEFER && dy == 2 && last_chunk) {
                    if (full_tile) load_old<COUT, C::MR, 4, true>(a, out_img, oy0, tx0 + lrow, cot * 64 + 4 * kg, old);
                    else load_old<COUT, C::MR, 4, false>(a, out_img, oy0, tx0 + lrow, cot * 64 + 4 * kg, old);
                }
                const unsigned char* Ab = Abuf + (chunk & 1) * C::A_BUF + (kg * C::NSLOT + slot_base + dy * C::IW) * 16;
                const unsigned char* Bb = Bbuf + (s & 1) * C::B_BUF + (kg * 64 + lrow) * 16;
                Frags fr[2];
#pragma unroll
                for (int k3 = 0; k3 < 3; ++k3) {
                    if constexpr (DEFER) {                    // units 2 (dy*3+k3) and +1: the 16 go out in the chunk's first 8 k-steps
                        if (qq == 0 && dy * 3 + k3 < C::MR * 2) { DEFER_UNIT(2 * (dy * 3 + k3)); DEFER_UNIT(2 * (dy * 3 + k3) + 1); }
                    }
                    if (k3 == 0) read_frags(fr[0], Ab, Bb, 0);
                    __builtin_amdgcn_sched_barrier(0);        // (this k-step's own fragments: in front of its MFMAs)
                    if (k3 == 0) {
                        if (ld_b) LOAD_B(rb[cur], (PEEL || q2 < Q) ? q2 : Q - 1, dy2);
                        if (ld_a) LOAD_A(ra[cur], qn + 1, dyn);
                    }
                    if (k3 < 2) read_frags(fr[(k3 + 1) & 1], Ab, Bb, k3 + 1);
                    if (k3 == 2) {
                        if (st_b) STORE_B((s + 1) & 1, rb[cur ^ 1]);
                        if (st_a) STORE_A((chunk + 1) & 1, dy, ra[cur ^ 1]);
                    }
                    const Frags& f = fr[k3 & 1];
#pragma unroll
                    for (int m = 0; m < C::MR; ++m)
#pragma unroll
                        for (int n = 0; n < 4; ++n) { MFMA3(acc[m][n], f.wh[n], f.wl[n], f.xh[m], f.xl[m]); }
                    // issue order: each MFMA followed by the fillers of its gap - fragment reads in the first 32 gaps (done well
                    // before the next k-step), global loads / LDS stores in the odd gaps
                    constexpr int NSTB = C::B_ITEMS, NSTG = C::B_ITEMS + 2 * C::A_ITEMS;   // global loads = LDS stores per stage
                    if (k3 == 0) {
                        if (ld_a) wide_interleave<16, NSTG, 0>();
                        else if (ld_b) wide_interleave<16, NSTB, 0>();
                        else wide_interleave<16, 0, 0>();
                    } else if (k3 == 1) {
                        wide_interleave<16, 0, 0>();
                    } else {
                        if (st_a) wide_interleave<0, 0, NSTG>();
                        else if (st_b) wide_interleave<0, 0, NSTB>();
                        else wide_interleave<0, 0, 0>();
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
            // ---- the 8-wave and lean forms (stage top, then three k-steps with their reads clustered in front of the MFMAs)
            // ---- land what was loaded one stage ago in the buffers of stage s+1 (free since the last barrier) -------
#define PIPE_LAND()                                                                                 \
            {                                                                                       \
                if (s + 1 < 3 * Q) STORE_B((s + 1) & 1, rb[RS(cur ^ 1)]);                            \
                if (q < C::NCHUNK - 1) STORE_A((chunk + 1) & 1, dy, ra[RS(cur ^ 1)]);                \
            }
            if constexpr (ONE_SET) { PIPE_LAND(); }
            // ---- issue the loads that are two stages ahead (consumed from registers during the NEXT stage) ----
            {   // weights of stage s+2
                const int q2 = dy == 0 ? q : q + 1, dy2 = (dy + 2) % 3;
                if (q2 < Q) LOAD_B(rb[RS(cur)], q2, dy2);
                // activations stored during stage s+1 = (qn, dyn): part dyn of chunk(qn)+1 (first output slice only)
                const int qn = dy == 2 ? q + 1 : q, dyn = (dy + 1) % 3;
                if (qn < C::NCHUNK - 1) LOAD_A(ra[RS(cur)], qn + 1, dyn);
            }
            // (bias: a few cached bytes.  The multi-slice kernels fetch it at the slice's LAST stage top - live for one stage
            // instead of six - which pays for the longer-lived old values below)
            if (DEFER ? (dy == 2 && last_chunk) : (dy == 0 && chunk == 0)) load_bias<COUT, 4>(a, cot * 64 + 4 * kg, bias);
            // old state values of this output slice, used after its last MFMA.  (Fetching them one or two stages earlier - the
            // DEFER kernels' `old` registers are free by then - was measured and is WORSE, 60.1 / 60.4 against 58.4 us: vmcnt is
            // in-order, so the next stage's wait for its weights also waits for these older, slower loads.)
            // The DEFER kernels fetch them SPREAD instead: unit (m, n) right after the previous slice's unit (m, n) has been
            // stored from the same registers, one float4 per lane and k-step over the slice's first chunk - the launch's 256
            // workgroups run in lockstep, and a whole slice's old values at one stage top are a 16 MB burst (~3 us of HBM time
            // in front of a 1.3 us stage); a few small loads per stage, a stage or more old when used, stall nobody.
            if (OUT_STATE && !DEFER && dy == 2 && last_chunk) {
                if (full_tile) load_old<COUT, C::MR, 4, true>(a, out_img, oy0, tx0 + lrow, cot * 64 + 4 * kg, old);
                else load_old<COUT, C::MR, 4, false>(a, out_img, oy0, tx0 + lrow, cot * 64 + 4 * kg, old);
            }

            if constexpr (!ONE_SET) { PIPE_LAND(); }
#undef PIPE_LAND

            // ---- 3 k-steps of MFMAs on the current buffers; fragments are double-buffered in registers: the reads
            //      of k-step k+1 are issued before the MFMAs of k-step k --------------------------------------------
            const unsigned char* Ab = Abuf + (chunk & 1) * C::A_BUF + (kg * C::NSLOT + slot_base + dy * C::IW) * 16;
            const unsigned char* Bb = Bbuf + (s & 1) * C::B_BUF + (kg * 64 + lrow) * 16;
            Frags fr[2];
            read_frags(fr[0], Ab, Bb, 0);
#pragma unroll
            for (int k3 = 0; k3 < 3; ++k3) {
                __builtin_amdgcn_sched_barrier(0);            // reads of k-step k3+1 stay ahead of the MFMAs of k3
                if (k3 < 2) read_frags(fr[(k3 + 1) & 1], Ab, Bb, k3 + 1);
                if constexpr (DEFER) {
                    if (qq == 0 && dy * 3 + k3 < C::MR * 4) DEFER_UNIT(dy * 3 + k3);
                }
                __builtin_amdgcn_sched_barrier(0);
                const Frags& f = fr[k3 & 1];
#pragma unroll
                for (int m = 0; m < C::MR; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) { MFMA3(acc[m][n], f.wh[n], f.wl[n], f.xh[m], f.xl[m]); }
            }
            }   // (the 8-wave and lean forms)

            // ---- output tile of this 64-channel slice ------------------------------------------------------------
            if (DEFER && dy == 2 && last_chunk && cot != C::NCOT - 1) {
#pragma unroll
                for (int m = 0; m < C::MR; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const float4 o = old[m][n];
                        old[m][n] = make_float4(o.x + a.sign * (acc[m][n][0] + bias[n].x), o.y + a.sign * (acc[m][n][1] + bias[n].y),
                                                o.z + a.sign * (acc[m][n][2] + bias[n].z), o.w + a.sign * (acc[m][n][3] + bias[n].w));
                        acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                pending = true;
                pend_cot = cot;
            } else if (dy == 2 && last_chunk) {
                if (full_tile) store_tile<COUT, OUT_STATE, C::MR, 4, true>(a, out_img, oy0, tx0 + lrow, cot * 64 + 4 * kg, acc, bias, old);
                else store_tile<COUT, OUT_STATE, C::MR, 4, false>(a, out_img, oy0, tx0 + lrow, cot * 64 + 4 * kg, acc, bias, old);
#pragma unroll
                for (int m = 0; m < C::MR; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (DEFER && qq == 0 && dy == 2) pending = false;       // the previous slice's eight units went out in this chunk
            __syncthreads();
        }
      }
    }
    }
#undef A_TABLE
#undef LOAD_A
#undef STORE_A
#undef LOAD_B
#undef STORE_B
#undef F4_
#undef RS
#undef DEFER_UNIT
    VST_TRACE_END_(4, CIN, COUT)
}

// Diagnostic fp32 direct convolution (VST_PREC_FP32): one thread per (pixel, co), plain FMA chain.
template <bool IN_STATE, bool OUT_STATE>
__global__ __launch_bounds__(256) void conv_fp32_kernel(const ConvArgs a, int CIN, int COUT, int STRIDE, int B) {
    const size_t total = (size_t)B * a.Hout * a.Wout * COUT;
    const float* wf = (const float*)a.packed;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int co = idx % COUT;
        size_t rest = idx / COUT;
        const int ox = rest % a.Wout; rest /= a.Wout;
        const int oy = rest % a.Hout;
        const int b = rest / a.Hout;
        const float* in_img = a.in + (size_t)b * a.in_img_stride;
        float acc = a.bias[co];
        for (int tap = 0; tap < 9; ++tap) {
            const int gy = reflect_clamp(oy * STRIDE - 1 + tap / 3, a.Hin);
            const int gx = reflect_clamp(ox * STRIDE - 1 + tap % 3, a.Win);
            const float* p = in_img + (IN_STATE ? zc_offset(vst_level_of_channels(CIN), gy, gx, a.Wq)
                                                : ((size_t)gy * a.Win + gx) * CIN);
            const float* w = wf + (size_t)tap * CIN * COUT + co;
            for (int ci = 0; ci < CIN; ++ci) acc = fmaf(p[ci], w[(size_t)ci * COUT], acc);
        }
        float* out_img = a.out + (size_t)b * a.out_img_stride;
        if (OUT_STATE) {
            float* p = out_img + zc_offset(vst_level_of_channels(COUT), oy, ox, a.Wq) + co;
            *p = *p + a.sign * acc;
        } else {
            out_img[((size_t)oy * a.Wout + ox) * COUT + co] = acc > 0.f ? acc : 0.f;
        }
    }
}
// ---- launches ---------------------------------------------------------------------------------------------------------
// Every MFMA conv kernel runs on a 1-D grid of round_up(tiles, 8) workgroups (xcd_tile) with its LDS as dynamic shared memory:
// this is the one place that sets the attribute, counts the tw x th tiles (times ncot output-channel tiles where the kernel
// does not loop them itself) and launches.  The kernel is a template argument, so every kernel function has its own
// "attribute already set" mask.
template <void (*KERN)(const ConvArgs)>
static int launch_tiles(int threads, int lds_bytes, int tw, int th, int ncot, int B, const ConvArgs& a, hipStream_t st) {
    static std::atomic<unsigned> attr_done{0};
    if (int rc = vst_ensure_dynamic_lds((const void*)KERN, lds_bytes, &attr_done)) return rc;
    ConvArgs t = a;
    t.tiles_x = (a.Wout + tw - 1) / tw; t.tiles_y = (a.Hout + th - 1) / th;
    t.tiles_total = t.tiles_x * t.tiles_y * B * ncot;
    const int grid = (t.tiles_total + 7) / 8 * 8;
    VST_TRACE_RESERVE(t, grid)
    KERN<<<dim3(grid), threads, lds_bytes, st>>>(t);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

// a stage-3 conv of the bf16x3 mode in one of conv_pipe_kernel's forms: see PipeCfg
template <int CIN, int COUT, bool IN_STATE, bool OUT_STATE, int NW, int MR>
static int launch_pipe(const ConvArgs& a, int B, hipStream_t st) {
    using C = PipeCfg<CIN, COUT, NW, MR>;
    return launch_tiles<conv_pipe_kernel<CIN, COUT, IN_STATE, OUT_STATE, NW, MR>>(C::NTHR, C::LDS_BYTES, 16, C::TH, 1, B, a, st);
}

template <int CIN, int COUT, int STRIDE, bool IN_STATE, bool OUT_STATE>
static int launch_conv(const ConvArgs& a, int B, int precision, hipStream_t st, bool out_h16 = false) {
    if (precision == VST_PREC_FP32) {
        const size_t total = (size_t)B * a.Hout * a.Wout * COUT;
        size_t blocks = (total + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        conv_fp32_kernel<IN_STATE, OUT_STATE><<<dim3((unsigned)blocks), 256, 0, st>>>(a, CIN, COUT, STRIDE, B);
        VST_RETURN_IF_LAUNCH_FAILED();
        return VST_OK;
    }
    if (precision != VST_PREC_BF16X3 && !vst_is_f16(precision)) return VST_E_MODE;
    vst_prof_scope prof(VST_KERNEL_ID(CIN, COUT, STRIDE), st);
    if constexpr (CIN >= 64 && COUT >= 64 && STRIDE == 1) {
        // VST_OPT_STAGE3_LEAN: half-CU workgroups; VST_OPT_STAGE3_WIDE: one wave per SIMD on the 16 x 16 tile; else two (8 waves)
        if (vst_option(VST_OPT_STAGE3_LEAN)) return launch_pipe<CIN, COUT, IN_STATE, OUT_STATE, 4, 2>(a, B, st);
        if (vst_option(VST_OPT_STAGE3_WIDE)) return launch_pipe<CIN, COUT, IN_STATE, OUT_STATE, 4, 4>(a, B, st);
        return launch_pipe<CIN, COUT, IN_STATE, OUT_STATE, 8, 2>(a, B, st);
    } else {
        using C = ConvCfg<CIN, COUT, STRIDE>;
        // f16x2: the convs of the 16- and 64-channel blocks run the 2-term fp16 product as well (one weight plane in LDS: one
        // more workgroup per CU, a third fewer MFMAs)
        constexpr bool T2_SHAPE = (CIN == 64 && COUT == 16) || (CIN == 16 && COUT == 16 && STRIDE == 2) || (CIN == 16 && COUT == 4);
        if constexpr (T2_SHAPE) {
            if (vst_is_f16(precision)) {
                if constexpr (!OUT_STATE) {                  // an h1 intermediate of a 16- / 64-channel block: fp16 on request
                    if (out_h16)
                        return launch_tiles<conv_mfma_kernel<CIN, COUT, STRIDE, IN_STATE, OUT_STATE, false, 2, true>>(
                            256, C::LDS_BYTES_T2, C::TW, C::TH, C::NCOT, B, a, st);
                }
                return launch_tiles<conv_mfma_kernel<CIN, COUT, STRIDE, IN_STATE, OUT_STATE, false, 2>>(
                    256, C::LDS_BYTES_T2, C::TW, C::TH, C::NCOT, B, a, st);
            }
        }
        if constexpr (CIN == 16 && COUT == 4 && STRIDE == 1 && !OUT_STATE) {
            if (vst_option(VST_OPT_STAGE1_FOLD))             // the tap-folded form: two k steps, same tiles
                return launch_tiles<conv_mfma_kernel<CIN, COUT, STRIDE, IN_STATE, OUT_STATE, false, 3, false, true>>(
                    256, ConvCfg<CIN, COUT, STRIDE, 0, 2>::LDS_BYTES, C::TW, C::TH, C::NCOT, B, a, st);
        }
        return launch_tiles<conv_mfma_kernel<CIN, COUT, STRIDE, IN_STATE, OUT_STATE, false, 3>>(
            256, C::LDS_BYTES, C::TW, C::TH, C::NCOT, B, a, st);
    }
}

// conv.1 of the stride-2 256-channel block with its output written as split planes (the F16X2 path)
static int launch_conv_s2_planes(const ConvArgs& a, int B, hipStream_t st) {
    using C = ConvCfg<64, 64, 2>;
    vst_prof_scope prof(VST_KERNEL_ID(64, 64, 2), st);
    // (the f16x2 path: 2-term fp16 like the rest of the block)
    return launch_tiles<conv_mfma_kernel<64, 64, 2, true, false, true, 2>>(256, C::LDS_BYTES_T2, C::TW, C::TH, C::NCOT, B, a, st);
}

// conv.4 + conv.7 of a 16- / 64-channel block on 16 x 16 tiles.  f16x2: the 2-term fp16 product; f16x2h: h1 arrives as fp16
// (launch_conv(..., out_h16 = true) wrote it)
template <int MID, int CH>
static int launch_pair(const ConvArgs& a, int B, int precision, hipStream_t st) {
    const bool t2 = vst_is_f16(precision), h16 = precision == VST_PREC_F16X2H;
    vst_prof_scope prof(VST_KERNEL_ID(MID, CH, 1), st);
    if constexpr (MID == 4) {
        if (a.rgb || a.rgb_u8) {                             // the last inverse block: the image instead of the state
            constexpr int LDS = PairCfg<MID, CH, 3>::LDS_BYTES;      // (the largest of the three forms' LDS, for all of them)
            static_assert(LDS >= PairCfg<MID, CH, 2>::LDS_BYTES && LDS >= PairCfg<MID, CH, 2, 4, true>::LDS_BYTES, "");
            if (h16) return launch_tiles<conv_pair_kernel<MID, CH, 2, 4, true, true>>(256, LDS, 16, 16, 1, B, a, st);
            if (t2) return launch_tiles<conv_pair_kernel<MID, CH, 2, 4, false, true>>(256, LDS, 16, 16, 1, B, a, st);
            return launch_tiles<conv_pair_kernel<MID, CH, 3, 4, false, true>>(256, LDS, 16, 16, 1, B, a, st);
        }
    }
    if (h16) return launch_tiles<conv_pair_kernel<MID, CH, 2, 4, true>>(256, PairCfg<MID, CH, 2, 4, true>::LDS_BYTES, 16, 16, 1, B, a, st);
    if (t2) return launch_tiles<conv_pair_kernel<MID, CH, 2>>(256, PairCfg<MID, CH, 2>::LDS_BYTES, 16, 16, 1, B, a, st);
    return launch_tiles<conv_pair_kernel<MID, CH, 3>>(256, PairCfg<MID, CH, 3>::LDS_BYTES, 16, 16, 1, B, a, st);
}

// one coupling block: dst (+/-)= F(src), three launches (h1, h2 are fp32 channels-last intermediates)
template <int CH, int STRIDE>
static int run_block(const vst_block_weights* w, int direction, int precision, float* dst, const float* src,
                     float* tmp, int B, int H, int W, hipStream_t st, float* rgb = nullptr, uint8_t* rgb_u8 = nullptr,
                     int rgb_c = 0) {
    constexpr int LV = CH == 16 ? 0 : (CH == 64 ? 1 : 2);
    constexpr int MID = CH / 4;
    constexpr int IN_CH = STRIDE == 1 ? CH : CH / 4;
    const int Ho = H >> LV, Wo = W >> LV;
    const size_t state_img = (size_t)H * W * 16;
    const size_t mid_img = (size_t)Ho * Wo * MID;
    float* h1 = tmp;
    float* h2 = tmp + (size_t)B * mid_img;
    ConvArgs a{};
    a.Wq = W >> 2;
    // conv.1: state -> h1 (ReLU)
    a.in = src; a.out = h1; a.packed = (const unsigned char*)w->conv[0].packed; a.bias = w->conv[0].bias;
    a.Hin = Ho * STRIDE; a.Win = Wo * STRIDE; a.Hout = Ho; a.Wout = Wo;
    a.in_img_stride = state_img; a.out_img_stride = mid_img; a.sign = 0.f;
    if constexpr (CH == 256 && STRIDE == 2) {
        if (vst_is_f16(precision)) {
            // the F16X2 path: h1 / h2 as split fp16 planes, conv.4 and conv.7 on conv3.hip's kernels.  In a forward pass the
            // new state half also goes out as planes: it is the src of the run of stride-1 blocks that follows.
            const size_t mid_bytes = (size_t)Ho * Wo * 64 * 4;
            unsigned char* const h1p = (unsigned char*)tmp;
            unsigned char* const h2p = h1p + (size_t)B * mid_bytes;
            unsigned char* const planes_a = h2p + (size_t)B * mid_bytes;
            a.out_sp = h1p; a.out_sp_img_bytes = mid_bytes;
            int rc2 = launch_conv_s2_planes(a, B, st);
            if (rc2) return rc2;
            const int h2_single = precision == VST_PREC_F16X2H;
            rc2 = vst3_conv_mid(&w->conv[1], h1p, h2p, h2_single, B, H, W, st);
            if (rc2) return rc2;
            return vst3_conv_out(&w->conv[2], h2p, h2_single, dst, direction > 0 ? planes_a : nullptr, direction > 0 ? 1.f : -1.f,
                                 B, H, W, st);
        }
    }
    // f16x2h: h1 of the 16- / 64-channel blocks goes through HBM as fp16 (the pair kernel that reads it is chosen by the same test)
    const bool h16 = CH <= 64 && precision == VST_PREC_F16X2H;
    int rc = launch_conv<IN_CH, MID, STRIDE, true, false>(a, B, precision, st, h16);
    if (rc) return rc;
    if constexpr (CH <= 64) {
        if (precision != VST_PREC_FP32) {         // conv.4 + conv.7 in one launch, h2 stays in LDS
            a.in = h1; a.out = dst; a.Hin = Ho; a.Win = Wo; a.in_img_stride = mid_img; a.out_img_stride = state_img;
            a.packed = (const unsigned char*)w->conv[2].packed; a.bias = w->conv[2].bias;
            a.packed1 = (const unsigned char*)w->conv[1].packed; a.bias1 = w->conv[1].bias;
            a.sign = direction > 0 ? 1.f : -1.f;
            a.rgb = rgb; a.rgb_u8 = rgb_u8; a.rgb_c = rgb_c;         // (block 0 of an inverse pass only: vst_block0_to_image)
            return launch_pair<MID, CH>(a, B, precision, st);
        }
    }
    // conv.4: h1 -> h2 (ReLU)
    a.in = h1; a.out = h2; a.packed = (const unsigned char*)w->conv[1].packed; a.bias = w->conv[1].bias;
    a.Hin = Ho; a.Win = Wo; a.in_img_stride = mid_img;
    rc = launch_conv<MID, MID, 1, false, false>(a, B, precision, st);
    if (rc) return rc;
    // conv.7: h2 -> dst += sign * (.)
    a.in = h2; a.out = dst; a.packed = (const unsigned char*)w->conv[2].packed; a.bias = w->conv[2].bias;
    a.out_img_stride = state_img; a.sign = direction > 0 ? 1.f : -1.f;
    return launch_conv<MID, CH, 1, false, true>(a, B, precision, st);
}

VST_DEFINE_TU_RANGE(vst_range_tu_conv)

int vst_block0_to_image(const vst_block_weights* w0, int precision, float* dst, const float* src, float* tmp, int B, int H,
                        int W, float* rgb, uint8_t* rgb_u8, int rgb_c, void* stream) {
    return run_block<16, 1>(w0, -1, precision, dst, src, tmp, B, H, W, (hipStream_t)stream, rgb, rgb_u8, rgb_c);
}

extern "C" {

// h1 + h2 (8 floats per pixel) + the split planes of both state halves for the stage-3 kernels of conv3.hip (2 x 16)
size_t vst_block_tmp_bytes(int B, int H, int W) { return (size_t)B * H * W * 40 * sizeof(float); }

int vst_block_apply(const vst_block_weights* w, int channel, int stride, int direction, int precision,
                    float* dst, const float* src, void* tmp, int B, int H, int W, void* stream) {
    if (!w || !dst || !src || !tmp) return VST_E_ARG;
    if (!vst_shape_ok(B, H, W)) return VST_E_SHAPE;
    if (direction != 1 && direction != -1) return VST_E_MODE;
    for (int i = 0; i < 3; ++i)
        if (!w->conv[i].packed || !w->conv[i].bias) return VST_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* t = (float*)tmp;
    if (channel == 16 && stride == 1) return run_block<16, 1>(w, direction, precision, dst, src, t, B, H, W, st);
    if (channel == 64 && stride == 1) return run_block<64, 1>(w, direction, precision, dst, src, t, B, H, W, st);
    if (channel == 64 && stride == 2) return run_block<64, 2>(w, direction, precision, dst, src, t, B, H, W, st);
    if (channel == 256 && stride == 1) {
        if (vst_is_f16(precision)) return vst3_block256(w, direction, precision, dst, src, tmp, -1, 0, B, H, W, stream);
        return run_block<256, 1>(w, direction, precision, dst, src, t, B, H, W, st);
    }
    if (channel == 256 && stride == 2) return run_block<256, 2>(w, direction, precision, dst, src, t, B, H, W, st);
    return VST_E_SHAPE;
}

}  // extern "C"
