/*
 * vstnet.h — C ABI of libvstnet_hip.so: the MI355X (gfx950) implementation of CAP-VSTNet's
 * inference hot path (RevResNet forward/inverse + cWCT).
 *
 * The reference (delldu/VSTNet) is pure Python on torch ops and defines no native interface for
 * this path; its closest native analogue is ggml's
 *     GGMLNetwork::engine_forward(int argc, TENSOR* argv[])   project/ggml/include/ggml_engine.h:610
 * Each entry point below names the reference Python symbol (file:line, relative to the reference
 * root) whose device work it replaces.  INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add in models/RevResNet.py / models/cWCT.py.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = VST_E_* (bad argument / unsupported shape),
 *     >0 = a hipError_t raised by a launch.  No exceptions cross the ABI.
 *   - all pointers are DEVICE pointers unless the name ends in _host; the library never allocates
 *     device memory: outputs and workspaces are caller-provided (vst_*_workspace_bytes tell sizes).
 *     The one exception is a segmentation plan (vst_seg_*, at the end), which owns its weights and workspaces.
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered and asynchronous.
 *     Entry points are re-entrant; use one stream per host thread / per GPU.
 *   - external tensors are NCHW fp32 contiguous (the reference's convention); H, W multiples of 4,
 *     H, W >= 8 (SURVEY.md 8(b) "Tensor conventions").
 *   - internal "state" buffers use the ZC layout described in DESIGN.md (quarter-resolution cells
 *     of 256 channels-last floats); they are opaque to callers of the whole-pass entry points.
 */
#ifndef VSTNET_H
#define VSTNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with hidden default visibility for its host code: exactly the declarations below are exported */
#pragma GCC visibility push(default)

#define VST_OK 0
#define VST_E_ARG (-1)      /* null pointer, non-positive size */
#define VST_E_SHAPE (-2)    /* H/W not multiple of 4, < 8, unsupported channel count */
#define VST_E_MODE (-3)     /* unknown precision / sp_steps / direction */
#define VST_E_WORKSPACE (-4)

/* conv arithmetic */
#define VST_PREC_BF16X3 0   /* bf16 MFMA, hi/lo split operands (3 products), fp32 accumulate: ~3e-6 rel */
#define VST_PREC_FP32 1     /* plain fp32 FMA direct convolution (diagnostic / cross-check, slow) */
#define VST_PREC_F16X2 2    /* fp16 MFMA, w_hi * (x_hi + x_lo): 2 products, activations split into fp16 hi + lo (22 bits),
                               weights rounded to fp16 once at pack time; in the 256-channel stride-1 blocks the
                               operands are pre-split in HBM and staged by LDS-DMA:
                               ~1.5e-4 rel on the code, ~4e-6 on a stylised frame */

#define VST_PREC_F16X2H 3   /* F16X2 with every conv input that crosses HBM taken as fp16 (11 bits) instead of fp16 hi + lo:
                               in the 256-channel blocks h1, h2 and the state as the first conv reads it (its hi plane;
                               the state itself keeps hi + lo) - one MFMA per product, half the bytes -, and h1 of the
                               16- and 64-channel blocks (2 bytes per value through HBM instead of 4):
                               ~1.75e-4 rel (1.94e-4 max) on the code, ~4e-5 (1.1e-4 max) on a stylised frame */

#define VST_NUM_BLOCKS 32   /* 30 stack blocks + 2 channel_reduction blocks */

int vst_version(void);
const char* vst_error_string(int code);

/* Largest frame of the whole-frame entry points: H * W <= VST_MAX_FRAME_PIXELS (2^26 = 8192 x 8192 pixels) per image; every
 * entry point that takes a frame shape returns VST_E_SHAPE past it, before it touches memory.  The bound is the 32-bit byte
 * offset of one image's split fp16 planes in the 256-channel blocks (64 B per pixel, csrc/common.h sp_offset); the other
 * per-image offsets (the state's 16 floats per pixel in 32 bits, ...) allow more, and image b of a batch starts at a 64-bit
 * base.  Larger frames: the halo-tiled driver (vstnet_amd/tiled.py, DESIGN.md "Ultra-resolution"), built on
 * vst_cwct_stats_code_rect / vst_cwct_stats_labels_code_rect below. */
#define VST_MAX_FRAME_PIXELS ((int64_t)1 << 26)
int64_t vst_max_frame_pixels(void);

/* ---------------------------------------------------------------------------------------------
 * Weights.  A residual_block (models/RevResNet.py:68-94) has three 3x3 convs (conv.1, conv.4,
 * conv.7).  vst_conv_packed_bytes/vst_pack_conv turn one OIHW fp32 weight tensor (device) into the
 * packed form the kernels read: [fp32 taps-major copy | bf16 hi fragments | bf16 lo fragments
 * | for cin, cout >= 64: fp16 fragments in the K order of the LDS-DMA kernels].
 * ------------------------------------------------------------------------------------------- */
size_t vst_conv_packed_bytes(int cout, int cin);
int vst_pack_conv(const float* w_oihw, int cout, int cin, void* packed, void* stream);

/* Exponent normalisation of one residual_block's intermediates (models/RevResNet.py:79-88): ReLU is positively homogeneous, so
 *   h1 = ReLU(W1 x + b1), h2 = ReLU(W4 h1 + b4), F = W7 h2 + b7
 * is unchanged by (W1, b1) *= s1 per output channel, W4 /= s1 per input channel, (W4, b4) *= s2 per output channel, W7 /= s2 per
 * input channel.  With s = 2^-round(log2 ||row||_2) (powers of two: exact in fp32, bit-identical results in the fp32-class
 * modes) every intermediate channel's weight row has unit scale, so h1 / h2 have the scale of the state whatever per-channel
 * scales a checkpoint was trained into, which is what the fp16 operand range of VST_PREC_F16X2 / F16X2H wants.  In place on
 * DEVICE copies of the five tensors (OIHW fp32 / [cout]); call before vst_pack_conv.  scales (optional) = float[2 * c_mid]
 * {s1, s2}.  c_mid <= 64. */
int vst_normalize_block(float* w1, float* b1, float* w4, float* b4, float* w7, int c_in1, int c_mid, int c_out,
                        float* scales, void* stream);

/* fp16 range flags of the narrowed modes, accumulated on the device since the last reset: */
#define VST_RANGE_SATURATED 1u /* an activation beyond +-65504 was clamped when it was rounded to fp16 (F16X2 / F16X2H) */
#define VST_RANGE_WEIGHT 2u    /* vst_pack_conv met a weight beyond +-65504 (its fp16 copy is +-Inf; BF16X3 / FP32 unaffected) */
/* *flags_host = OR of the flags raised on the current device; reset != 0 clears them.  Synchronises the device (a calibration
 * / diagnostic call: RevResNet.check_range, bench.py, tests), never called by the passes themselves. */
int vst_range_flags(unsigned* flags_host, int reset);
/* the same without synchronising: four words (their OR = the flags) copied to DEVICE memory in stream order - a frame loop
 * appends them to the frame's own D2H copy and looks at them when it retires the frame (vstnet_amd/pipeline.py) */
int vst_range_flags_async(unsigned* flags4_dev, void* stream);

typedef struct vst_conv_weights {
    const void* packed;   /* from vst_pack_conv */
    const float* bias;    /* [cout] fp32 */
} vst_conv_weights;

typedef struct vst_block_weights {
    vst_conv_weights conv[3];
} vst_block_weights;

/* blocks[0..29] = stack.0..29, blocks[30..31] = channel_reduction.block_list.0..1 (host struct of
 * device pointers; models/RevResNet.py:190,192-201) */
typedef struct vst_net_weights {
    vst_block_weights blocks[VST_NUM_BLOCKS];
} vst_net_weights;

/* ---------------------------------------------------------------------------------------------
 * Layout glue (R-1..R-3 of SURVEY.md 8(a)): split/merge, injective_pad, squeeze/unsqueeze are
 * address arithmetic in the ZC state layout; only the NCHW boundary needs data movement.
 * state halves s1,s2: [B][H/4][W/4][256] fp32 each.
 * ------------------------------------------------------------------------------------------- */
/* x[B,C,H,W] (C<=16) -> s1 (channels C..15 zero), s2 = 0.   inj_pad.forward + split, RevResNet.py:212-214 */
int vst_pack_input(const float* x, float* s1, float* s2, int B, int C, int H, int W, void* stream);
/* s1 -> x[B,C,H,W]: merge + inj_pad.inverse, RevResNet.py:235-237 */
int vst_unpack_output(const float* s1, float* x, int B, int C, int H, int W, void* stream);
/* uint8 frame edge: frames_hwc[B,H,W,3] -> s1/s2 with ToTensor scaling (u8/255, image_transfer.py:167)
 * and back with mul(255).clamp(0,255).byte() truncation (image_transfer.py:217-218) */
int vst_pack_input_u8(const uint8_t* frames_hwc, float* s1, float* s2, int B, int H, int W, void* stream);
int vst_unpack_output_u8(const float* s1, uint8_t* frames_hwc, int B, int H, int W, void* stream);
/* Lab luminance-preserving post-process of the fork: out = lab2rgb(cat(L(content),
 * ab(clamp(stylized,0,1)))), all three [B,3,H,W] fp32 in [0,1]; any H, W >= 1 (no multiple-of-4 requirement).
 * project/image_style/vstnet.py:189-220, project/image_style/color.py:18-113.  out may alias stylized. */
int vst_lab_luminance(const float* content, const float* stylized, float* out, int B, int H, int W, void* stream);
/* The same blend at the uint8 frame edge of the video loop (vstnet_amd/pipeline.py): content_hwc = the uint8 frame [B][H][W][3]
 * the loop already holds on the device, read as u8 / 255.f (a true division, like vst_pack_input_u8); stylized = fp32 planes
 * [B][3][H][W], what vst_revnet_decode / _decode_labels / _inverse write.  _u8: out_hwc[B][H][W][3] = the blend * 255, clamped to
 * [0, 255], truncated (the quantisation of vst_unpack_output_u8): 18 B per pixel.  _u8_f32: the blend as fp32 planes for a resize
 * to the writer size that follows it (out may alias stylized).  Replaces, per frame, the fork's rgb2lab / rgb2lab / lab2rgb
 * (project/image_style/vstnet.py:189-220, color.py:18-113) and the reference's ToTensor and mul(255).clamp(0,255).byte()
 * (video_transfer.py:188,212).  Any H, W >= 1.  VST_E_ARG for a null pointer; VST_E_SHAPE for B <= 0, H * W past
 * VST_MAX_FRAME_PIXELS or B > 65535; checks come before any launch. */
int vst_lab_luminance_u8(const uint8_t* content_hwc, const float* stylized, uint8_t* out_hwc, int B, int H, int W, void* stream);
int vst_lab_luminance_u8_f32(const uint8_t* content_hwc, const float* stylized, float* out, int B, int H, int W, void* stream);
/* merge + "spread" (unsqueeze x sp_steps), RevResNet.py:139-144 -> z[B,32,H,W] (sp=2) or [B,128,H/2,W/2] (sp=1) */
int vst_spread(const float* s1, const float* s2, float* z, int B, int H, int W, int sp_steps, void* stream);
/* inverse of vst_spread: squeeze x sp_steps + split, RevResNet.py:148-154 */
int vst_gather(const float* z, float* s1, float* s2, int B, int H, int W, int sp_steps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One coupling block, in place on the state (R-4/R-5; residual_block.forward RevResNet.py:96-104,
 * .inverse :106-116):   direction=+1:  dst += F(src)      direction=-1:  dst -= F(src)
 * `channel` in {16,64,256}, `stride` in {1,2} (stride 2: src is read at the finer resolution).
 * tmp must hold vst_block_tmp_bytes(B,H,W) bytes.
 * ------------------------------------------------------------------------------------------- */
size_t vst_block_tmp_bytes(int B, int H, int W);
int vst_block_apply(const vst_block_weights* w, int channel, int stride, int direction, int precision,
                    float* dst, const float* src, void* tmp, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole passes (R-6/R-7): RevResNet._forward RevResNet.py:210-223 and ._inverse :225-239.
 * workspace: vst_pass_workspace_bytes(B,H,W).
 * workspace: 256-byte aligned, as every allocator here returns it.
 * ------------------------------------------------------------------------------------------- */
size_t vst_pass_workspace_bytes(int B, int H, int W);
/* images per internal sub-batch of vst_revnet_forward / _inverse for this shape (the passes keep a sub-batch's working set
 * inside the 256 MiB Infinity Cache); 1 = the passes run image by image.  < 0: VST_E_SHAPE. */
int vst_pass_sub_batch(int B, int H, int W);
int vst_revnet_forward(const vst_net_weights* w, const float* x, float* z, void* workspace,
                       int B, int C_in, int H, int W, int sp_steps, int precision, void* stream);
int vst_revnet_inverse(const vst_net_weights* w, const float* z, float* x, void* workspace,
                       int B, int C_out, int H, int W, int sp_steps, int precision, void* stream);

/* the same passes with the uint8 HWC frame edge fused into the boundary kernels (video_transfer.py:188,210-214) */
int vst_revnet_forward_u8(const vst_net_weights* w, const uint8_t* frames_hwc, float* z, void* workspace,
                          int B, int H, int W, int sp_steps, int precision, void* stream);
int vst_revnet_inverse_u8(const vst_net_weights* w, const float* z, uint8_t* frames_hwc, void* workspace,
                          int B, int H, int W, int sp_steps, int precision, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Packed code.  The reference's forward pass ends with merge + unsqueeze steps (RevResNet.py:139-144, :219-222) that only
 * permute (channel, pixel) pairs, and its inverse starts by undoing them (:148-154, :228-231); an unmasked cWCT
 * (cWCT.py:24-47, :206-262) is indifferent to the order of the pixels.  So the code can stay in the layout the coupling
 * blocks leave it in: `code` = float[B][2 halves][H/4][W/4][256] (the same number of floats as z), i.e. one row of N floats
 * per code pixel: sp_steps = 2 (photorealistic, N = 32): cell (h,w) of half i holds the rows of the pixels
 * (4h+2i+i', 4w+2j+j') in the order (j, i', j'); sp_steps = 1 (artistic, N = 128, z = [B,128,H/2,W/2]): the rows of the
 * pixels (2h+i, 2w+j), j = 0, 1.
 *   vst_revnet_encode[_u8] : forward pass without the spread; the state halves are written straight into `code`
 *                            (the same for both modes).
 *   vst_revnet_decode[_u8] : inverse pass without the gather.  `affines` (NULL, or float[B][N*N+N] as produced by
 *                            vst_cwct_factor): y = T x + t0 is applied to every row of image b first - the cWCT of
 *                            that frame - while the state is loaded (`code` itself is not modified).
 *   vst_code_to_z / vst_z_to_code : the permutation itself (z <-> code), for callers that want to look at z.
 *   vst_cwct_stats_code    : vst_cwct_stats (all pixels, no mask) of ONE image's code; same stats record.
 *   vst_cwct_apply_code    : y = T x + t0 on one image's code, out of place or in place (out may alias code).
 * workspace: vst_pass_workspace_bytes(1,H,W) for the passes (images are processed one at a time),
 * vst_cwct_stats_code_workspace_bytes(H,W,sp_steps) for the statistics (vst_cwct_stats_labels_code_workspace_bytes(H,W) for
 * the per-label ones).
 * workspace: 256-byte aligned, as every allocator here returns it.
 * ------------------------------------------------------------------------------------------- */
int vst_revnet_encode(const vst_net_weights* w, const float* x, float* code, void* workspace,
                      int B, int C_in, int H, int W, int precision, void* stream);
int vst_revnet_encode_u8(const vst_net_weights* w, const uint8_t* frames_hwc, float* code, void* workspace,
                         int B, int H, int W, int precision, void* stream);
int vst_revnet_decode(const vst_net_weights* w, const float* code, const float* affines, float* x, void* workspace,
                      int B, int C_out, int H, int W, int sp_steps, int precision, void* stream);
int vst_revnet_decode_u8(const vst_net_weights* w, const float* code, const float* affines, uint8_t* frames_hwc,
                         void* workspace, int B, int H, int W, int sp_steps, int precision, void* stream);
int vst_code_to_z(const float* code, float* z, int B, int H, int W, int sp_steps, void* stream);
int vst_z_to_code(const float* z, float* code, int B, int H, int W, int sp_steps, void* stream);
size_t vst_cwct_stats_code_workspace_bytes(int H, int W, int sp_steps);
int vst_cwct_stats_code(const float* code, int H, int W, int sp_steps, double* stats, void* workspace, void* stream);
int vst_cwct_apply_code(const float* code, float* out, int H, int W, int sp_steps, const float* affine, void* stream);
/* Masked transfer (cWCT.py:49-109) on ONE image's packed code (photorealistic codes, sp_steps = 2, only).  `mask_rows` = the label of every row, i.e. the [H][W] label
 * map in the code's pixel order (vst_mask_to_code; once per mask).  plan / max_slots / affines as in the vst_cwct_*_labels
 * calls below (vst_label_plan works on the label maps in any order); the apply and the decode take at most 8 slots
 * (VST_E_SHAPE otherwise: use the z route), the statistics any number.  Rows whose label has no slot keep their values. */
int vst_mask_to_code(const uint8_t* mask, uint8_t* mask_rows, int H, int W, void* stream);
size_t vst_cwct_stats_labels_code_workspace_bytes(int H, int W);
int vst_cwct_stats_labels_code(const float* code, int H, int W, const uint8_t* mask_rows, const void* plan, int max_slots,
                               double* stats, void* workspace, void* stream);
int vst_cwct_apply_labels_code(const float* code, float* out, int H, int W, const float* affines, const uint8_t* mask_rows,
                               const void* plan, int max_slots, void* stream);
/* Statistics of a pixel rectangle of ONE image's packed code: the records of vst_cwct_stats_code / _labels_code over the rows
 * whose pixels lie in [y0, y0 + h) x [x0, x0 + w) (image pixels; the rows map to pixels as in vst_mask_to_code).  A tile of a
 * larger frame takes the statistics of its interior this way; the halo belongs to its neighbours.  VST_E_ARG for a rectangle
 * that is empty or leaves the image, or (sp_steps = 1, whose rows are 2 x 2 pixels) has an odd origin or size.  The full
 * rectangle runs exactly vst_cwct_stats_code / _labels_code (bit-identical records).  Workspaces as for those calls. */
int vst_cwct_stats_code_rect(const float* code, int H, int W, int sp_steps, int y0, int x0, int h, int w, double* stats,
                             void* workspace, void* stream);
int vst_cwct_stats_labels_code_rect(const float* code, int H, int W, int y0, int x0, int h, int w, const uint8_t* mask_rows,
                                    const void* plan, int max_slots, double* stats, void* workspace, void* stream);
int vst_revnet_decode_labels(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                             const void* plan, int max_slots, float* x, void* workspace, int C_out, int H, int W,
                             int precision, void* stream);
int vst_revnet_decode_labels_u8(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                                const void* plan, int max_slots, uint8_t* frame_hwc, void* workspace, int H, int W,
                                int precision, void* stream);
/* Strength maps (version 109): a per-pixel blend between the code x and its cWCT A(x) = T x + t0, the map form of the
 * reference's alpha_c (which is linear in A: (1-a) A(x) + a x).  For the row of code pixel p with strength s = s(p) in [0, 1]
 * and every channel n:   d = A(x)[n] - x[n];   y[n] = (s == 1.0f) ? A(x)[n] : x[n] + s * d,   every operation rounded to fp32,
 * no FMA contraction.  s = 0 keeps x and s = 1 gives A(x), bit for bit; rows whose label has no slot keep x as before.
 * vst_map_to_code   : a float map at the CODE's resolution -> `rows`, one float per row in the packed code's row order:
 *                     sp_steps = 2: map [H][W], the order of vst_mask_to_code; sp_steps = 1: map [H/2][W/2], one value per
 *                     row of 128 ("Packed code" above).
 * vst_cwct_apply_code_blend / vst_cwct_apply_labels_code_blend / vst_revnet_decode_blend[_u8] /
 * vst_revnet_decode_labels_blend[_u8] : the calls of the same names without _blend, plus `strength_rows` (of ONE image for the
 *                     apply and the labels calls; float[B][rows] for vst_revnet_decode_blend[_u8], rows = H*W or H*W/4).  The
 *                     blend runs inside the apply kernels, before the store / the fp16 split.  NULL: exactly the plain call
 *                     (which is what the plain entry points pass).  Without affines there is nothing to blend.
 * vst_cwct_blend    : the dense NCHW routes, any N = 1..256: out[n][p] from x[n][p] (the code), y[n][p] (its cWCT) and
 *                     strength[p], p < L; out may alias x or y.  16-byte accesses when x, y and out are 16-byte aligned. */
int vst_map_to_code(const float* map, float* rows, int H, int W, int sp_steps, void* stream);
int vst_cwct_apply_code_blend(const float* code, float* out, int H, int W, int sp_steps, const float* affine,
                              const float* strength_rows, void* stream);
int vst_cwct_apply_labels_code_blend(const float* code, float* out, int H, int W, const float* affines, const uint8_t* mask_rows,
                                     const void* plan, int max_slots, const float* strength_rows, void* stream);
int vst_revnet_decode_blend(const vst_net_weights* w, const float* code, const float* affines, const float* strength_rows,
                            float* x, void* workspace, int B, int C_out, int H, int W, int sp_steps, int precision, void* stream);
int vst_revnet_decode_blend_u8(const vst_net_weights* w, const float* code, const float* affines, const float* strength_rows,
                               uint8_t* frames_hwc, void* workspace, int B, int H, int W, int sp_steps, int precision,
                               void* stream);
int vst_revnet_decode_labels_blend(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                                   const void* plan, int max_slots, const float* strength_rows, float* x, void* workspace,
                                   int C_out, int H, int W, int precision, void* stream);
int vst_revnet_decode_labels_blend_u8(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                                      const void* plan, int max_slots, const float* strength_rows, uint8_t* frame_hwc,
                                      void* workspace, int H, int W, int precision, void* stream);
int vst_cwct_blend(const float* x, const float* y, const float* strength, float* out, int N, long L, void* stream);
/* Style maps (version 112): a per-pixel mix of K = 2..8 styles, the map form of the reference's alpha_s.  `interpolation`
 * (models/cWCT.py:206-262) whitens once and mixes the colourings linearly, so for weights that sum to 1 it equals
 * sum_k a_k A_k(c) with A_k = T_k x + t0_k the affine map of style k alone at the same alpha_c; weights w_k(p) per code pixel
 * generalise that.  For the row of code pixel p and every channel n:
 *     a_k = A_k(x)[n]  exactly as the plain apply of that route computes it (the same MFMA sequence from a zero accumulator, + t0);
 *     m = w_0(p) * a_0;   m = m + w_k(p) * a_k  for k = 1 .. K-1 in this order;
 *     y[n] = m, or with strength_rows the strength blend of (x[n], m, s(p)) above;
 * every operation rounded to fp32, no FMA contraction; the mix comes before the strength blend and both before the fp16 split
 * of the f16x2 modes.  A one-hot row gives that style's A_k(x) (up to the sign of a zero), constant weights `interpolation`.
 * vst_cwct_apply_code_mix : vst_cwct_apply_code_blend on affines = float[K][N*N+N] and weight_rows = float[K][rows] (K planes in
 *                     the rows' order, each made by vst_map_to_code); strength_rows is nullable.  sp_steps = 1 (rows of 128)
 *                     holds two sets of fragments in LDS and takes K = 2 only.
 * vst_revnet_decode_mix[_u8] : vst_revnet_decode_blend[_u8] with affines = float[B][K][N*N+N], weight_rows = float[B][K][rows].
 * vst_cwct_mix_acc  : the dense NCHW routes, any N = 1..256: out[n][p] = first ? w[p] * a[n][p] : out[n][p] + w[p] * a[n][p],
 *                     p < L; K plain applies into one buffer with one call after each give the sum above.  out may alias a.
 *                     16-byte accesses when a and out are 16-byte aligned.
 * VST_E_ARG: K outside 2..8, a null pointer (strength_rows excepted), code / out / affines not 16-byte aligned, a float array
 * not 4-byte aligned; VST_E_MODE: sp_steps, or sp_steps = 1 with K != 2; VST_E_SHAPE: H, W, N, L.  Checks come before any GPU call. */
int vst_cwct_apply_code_mix(const float* code, float* out, int H, int W, int sp_steps, const float* affines, int K,
                            const float* weight_rows, const float* strength_rows, void* stream);
int vst_revnet_decode_mix(const vst_net_weights* w, const float* code, const float* affines, int K, const float* weight_rows,
                          const float* strength_rows, float* x, void* workspace, int B, int C_out, int H, int W, int sp_steps,
                          int precision, void* stream);
int vst_revnet_decode_mix_u8(const vst_net_weights* w, const float* code, const float* affines, int K, const float* weight_rows,
                             const float* strength_rows, uint8_t* frames_hwc, void* workspace, int B, int H, int W, int sp_steps,
                             int precision, void* stream);
int vst_cwct_mix_acc(const float* a, const float* w, float* out, int N, long L, int first, void* stream);
/* One frame's strength map, made on the device (version 110): a clip with one matte per frame and / or a strength per label of
 * the frame's own label map.  One launch on `stream`, no host synchronisation, nothing allocated.
 *   matte  (nullable) uint8 [H][W] grey at the stylised frame size;  labels (nullable) uint8 [H][W] at that size;
 *   table  256 floats in [0, 1], required when labels != NULL;
 *   dense  (nullable) float [cH][cW] in image order - what vst_cwct_blend reads;
 *   rows   (nullable) one float per packed row - what vst_map_to_code makes of `dense`, the same values in the other order.
 * sp_steps = 2: the code grid is the frame grid; sp_steps = 1: it is H/2 x W/2.  At least one input and one output.
 * Arithmetic (fp32, every operation rounded, no contraction):
 *   matte  sp_steps = 2: m = float(v) / 255.0f (a true division);  sp_steps = 1: Pillow's Image.BOX 2 x 2 on the 8-bit data
 *          first - two rounded passes, horizontal first: h = (a + b + 1) >> 1, v = (h_top + h_bottom + 1) >> 1 - then / 255;
 *   labels sp_steps = 2: t = table[label];  sp_steps = 1: t = ((t00 + t01) + (t10 + t11)) * 0.25f over the 2 x 2 block;
 *   s = m, s = t, or with both s = m * t.
 * A frame's matte so gives the rows that the host route (8-bit grey, BOX for artistic codes, / 255, vst_map_to_code) gives.
 * VST_E_ARG: neither input, neither output, labels without a table, a byte map or the table not 4-byte aligned, dense / rows not
 * 16-byte aligned; VST_E_SHAPE: H, W (multiples of 4, >= 8, H * W <= VST_MAX_FRAME_PIXELS); VST_E_MODE: sp_steps.  Checks come
 * before any GPU call. */
int vst_strength_frame(const uint8_t* matte, const uint8_t* labels, const float* table, float* dense, float* rows, int H, int W,
                       int sp_steps, void* stream);
/* Style maps per frame (version 120): one frame's style map, made on the device from the frame's 8-bit weight planes - a clip
 * whose style regions move.  One launch on `stream`, no host synchronisation, nothing allocated.
 *   planes   uint8 [n_planes][H][W] grey at the stylised frame size, contiguous.  n_planes = 1: the ramp between two styles,
 *            K = 2;  n_planes = 2..8: one plane per style, K = n_planes.
 *   dense    (nullable) float [K][cH * cW], every plane in image order - what vst_cwct_mix_acc reads;
 *   rows     (nullable) float [K][rows], every plane in the order vst_map_to_code gives - the weight_rows of the mix calls;
 *   flags    (nullable) one int the caller clears: bit 0 (VST_STYLE_FRAME_ZERO_SUM) is set - a vector atomic OR, at most one per
 *            wave, issued only by waves that saw such a pixel - when every plane is 0 at some code pixel.
 * sp_steps = 2: the code grid is the frame grid; sp_steps = 1: it is H/2 x W/2 (cH * cW = rows in both).
 * Arithmetic (fp32, every operation rounded, no contraction), per plane k and code pixel:
 *   u_k      sp_steps = 2: the byte v_k;  sp_steps = 1: Pillow's Image.BOX 2 x 2 on the 8-bit data - two rounded passes,
 *            horizontal first: h = (a + b + 1) >> 1, u = (h_top + h_bottom + 1) >> 1 (vst_strength_frame's);
 *   n_planes = 1:  t = float(u_0) / 255.0f (a true division);  w_0 = 1.0f - t;  w_1 = t;
 *   n_planes >= 2: total = sum_k u_k in integers;  w_k = float(u_k) / float(total);
 *            total == 0:  w_0 = 1.0f, w_k = 0.0f for k > 0, and the flag bit: no NaN reaches the decoder.
 * The planes so give the maps of the host route (8-bit grey, BOX for artistic codes, utils.style_map_weights, vst_map_to_code).
 * VST_E_ARG: planes NULL, neither output, n_planes outside 1..8, planes or flags not 4-byte aligned, dense / rows not 16-byte
 * aligned; VST_E_SHAPE: H, W (multiples of 4, >= 8, H * W <= VST_MAX_FRAME_PIXELS); VST_E_MODE: sp_steps.  sp_steps = 1 with
 * K > 2 is no error here: the dense route takes those maps.  Checks come before any GPU call. */
#define VST_STYLE_FRAME_ZERO_SUM 1
int vst_style_frame(const uint8_t* planes, int n_planes, float* dense, float* rows, int* flags, int H, int W, int sp_steps,
                    void* stream);
/* Statistics window (version 113): the content statistics of a video frame pooled with those of the
 * frames before it, so that the affine map - global to the frame - does not move with every change of the frame's content.
 * Every statistics call of this header writes the record double[1 + N + N*N] = {n, mean, cov} and every factor call reads it;
 * this call sits between the two.  One launch on `stream` (one workgroup per record), nothing allocated, no synchronisation.
 *   records_host_array[a], a = 0 .. n_ages - 1: a HOST array of DEVICE pointers; age 0 is the current frame, age a the frame a
 *           steps before it; each points at n_records consecutive raw records (1 = an unmasked frame, up to 32 = the slot
 *           table of the masked routes).  weights_host[a] > 0: the weight of age a (HOST).  Both travel in the kernel arguments.
 *   out     n_records records, overlapping no input (inputs may repeat);  used  int[n_records], may be NULL.
 * Arithmetic, all fp64, every record r on its own, every operation rounded (no contraction), all sums in increasing age:
 *   usable  age a is usable iff n_a >= 2 (a prefactored record has n < 0: not usable).
 *   scan    ages 1, 2, ... in order; an unusable age is skipped and does not stop the scan; with cut > 0 the first usable age
 *           with |mu_a - mu_0|^2 + |C_a - C_0|_F > cut * tr(C_0) ends it: that age and every older one are left out (a scene
 *           cut: nothing from before it reaches the frames after it).  cut = 0: no test.
 *   set     S = age 0 plus the usable ages the scan accepted; used[r] = |S|, or 0 if age 0 is unusable.
 *   copy    age 0 unusable, or S = {0}: out is a BIT copy of the age-0 record.
 *   pooled  otherwise, with m_a = w_a n_a:  M = sum m_a;  mu = (sum m_a mu_a) / M;
 *           S = sum w_a ((n_a - 1) C_a + (n_a (mu_a - mu)) (mu_a - mu)^T);  out = {M, mu, S / (M - 1)}.
 *           With equal weights that is the mean and (n - 1)-normalised covariance of the union of the frames' pixels: what the
 *           reference's whitening computes on the concatenated codes (models/cWCT.py:134-149).  Weights are the caller's: M - 1
 *           must come out positive (w_0 = 1, as decay ** age gives, always does).
 * VST_E_SHAPE: n_ages outside 1..VST_STATS_POOL_MAX, n_records outside 1..32, N outside 1..256.  VST_E_ARG: a null pointer
 * (used excepted), a record pointer or out not 8-byte aligned, a weight that is not positive and finite, cut negative or not
 * finite, out overlapping an input.  Every check comes before any launch.  The launch is profiled as VST_KERNEL_CWCT_POOL. */
#define VST_STATS_POOL_MAX 8
int vst_cwct_stats_pool(const double* const* records_host_array, const double* weights_host, int n_ages, int n_records, int N,
                        double cut, double* out, int* used, void* stream);
/* Statistics window by label (version 114): the same pool for frames whose label plans differ - the
 * per-frame plans of vst_label_plan_hists, whose slot sets and slot order change from frame to frame.  Records line up by the
 * LABEL a slot holds, not by the slot's number.  One launch on `stream` of max_slots workgroups, nothing allocated, no
 * synchronisation, no atomics.
 *   records_host_array[a], weights_host[a], cut, used: as above; every age is a block of max_slots consecutive raw records.
 *   plans_host_array[a]: a HOST array of DEVICE pointers to the plan (VST_LABEL_PLAN_BYTES) that age's records were reduced
 *           under; read on `stream`: whoever wrote it must be ordered before this call.
 *   out     max_slots records in the slot order of plans[0], overlapping no input;  used  int[max_slots], may be NULL.
 * Per slot r < max_slots:
 *   dead    r >= min(plans[0]->n_slots, max_slots): used[r] = 0 and record r of out is NOT written (nor is record r of any input read: a
 *           statistics call of max_slots = 8 never wrote those of its [32] block).
 *   key     L = plans[0]->slot_label[r].  For every age a >= 1 the record of L is the one at slot s < plans[a]->n_slots with
 *           plans[a]->slot_label[s] == L.  (The search ends at n_slots: slot_label is zero-padded and label 0 is a legal key;
 *           and at max_slots, the records an age's block holds.)
 *           No such slot: the age is unusable for this record - skipped, it does not stop the scan, like n_a < 2.
 *   then    usable, scan, set, copy and pooled exactly as above on the records so found, operation for operation: with the same
 *           plan at every age, out and used are those of vst_cwct_stats_pool bit for bit.
 * VST_E_SHAPE and VST_E_ARG as above (max_slots for n_records), and VST_E_ARG for a plan pointer that is null or not 4-byte
 * aligned.  Every check comes before any launch.  The launch is profiled as VST_KERNEL_CWCT_POOL. */
int vst_cwct_stats_pool_keyed(const double* const* records_host_array, const void* const* plans_host_array,
                              const double* weights_host, int n_ages, int max_slots, int N, double cut, double* out, int* used,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * cWCT (C-1..C-6; models/cWCT.py).  Feature matrices are x[N][L] fp32 row-major (one NCHW image:
 * N channels, L = H*W).  `mask` (optional, may be NULL) is uint8[L]; with a mask only pixels whose
 * label == `label` take part.
 *
 * vst_cwct_stats  : mean and covariance  C = Xc Xc^T/(n-1)  (cWCT.py:138-144,153-157), two-level
 *                   shifted accumulation, final combine in fp64.  stats = double[1 + N + N*N]:
 *                   {n, mean[N], cov[N*N]}.
 * vst_cwct_factor : builds the affine map of one (content,style) pair from their stats:
 *                   Lc = chol(Cc), Ls_i = chol(Cs_i) with the cumulative-jitter retry of
 *                   cholesky_dec (cWCT.py:111-132), mixL = sum_i alpha_i Ls_i (+ alpha_c blend,
 *                   cWCT.py:231-254), T = mixL * Lc^-1, t0 = mix_mean - T*mean_c.
 *                   affine = float[N*N + N] {T, t0};  info = int[2 + n_styles], IN/OUT: on entry the minimum
 *                   number of retries to start from (zeros normally; the reference factors a whole
 *                   [B,N,N] batch at once, cWCT.py:122-128, so a failing sample jitters every sample: a
 *                   caller reproduces that by a second call with the batch maximum), on exit
 *                   {content retries, overflow flag, style retries...}.
 * vst_cwct_apply  : y[:,p] = T x[:,p] + t0  (cWCT.py:147,161-162 fused); with a mask only pixels
 *                   whose label matches are written (in place allowed: y may alias x).
 * workspace: 256-byte aligned, as every allocator here returns it (vst_cwct_stats_workspace_bytes,
 * vst_cwct_labels_workspace_bytes).
 * ------------------------------------------------------------------------------------------- */
size_t vst_cwct_stats_workspace_bytes(int N, long L);
int vst_cwct_stats(const float* x, int N, long L, const uint8_t* mask, int label,
                   double* stats, void* workspace, void* stream);
int vst_cwct_factor(const double* content_stats, const double* const* style_stats_host_array,
                    const float* alphas_host, int n_styles, float alpha_c, float eps, int N,
                    float* affine, int* info, void* stream);
int vst_cwct_apply(const float* x, float* y, int N, long L, const float* affine,
                   const uint8_t* mask, int label, void* stream);
/* the same with the arithmetic chosen by the caller: VST_PREC_FP32 = exact-fp32 matrix-core / FMA kernels for every N,
 * shape and mask; otherwise (the default of vst_cwct_apply) unmasked N >= 64 applies with L % 64 == 0 run on bf16 MFMA
 * with split operands (3 products, ~1.5e-5 max-rel) and everything else is exact fp32 */
int vst_cwct_apply_prec(const float* x, float* y, int N, long L, const float* affine,
                        const uint8_t* mask, int label, int precision, void* stream);
/* ---- single-pass masked transfer (cWCT._transfer_seg, models/cWCT.py:49-109; compute_label_info :166-189) ----------------
 * vst_label_plan        : histograms both uint8 label maps ON THE DEVICE, applies the validity rule (count_c > 10, count_s > 10,
 *                         ratio < 100 both ways, cWCT.py:178) and gives the valid labels consecutive "slots" in increasing label
 *                         order (at most 32; more sets plan.overflow and keeps the content feature there).  plan = device buffer
 *                         of VST_LABEL_PLAN_BYTES: {int n_slots, overflow; int hist_c[256], hist_s[256]; u8 lut[256]; u8 slot_label[32]}.
 * vst_cwct_stats_labels : {n, mean, cov} of every slot in ONE pass over x (pixels of a tile are sorted by slot in LDS);
 *                         stats = double[32][1 + N + N*N].  N in {32, 64, 128}.  workspace: vst_cwct_labels_workspace_bytes.
 * vst_cwct_factor_labels: one workgroup per slot: affines[slot] = {T, t0} of (content slot, style slot); info = int[32][3].
 * vst_cwct_apply_labels : y[:,p] = T[slot(p)] x[:,p] + t0[slot(p)], y = x where the label has no slot; one pass (y may alias x).
 *                         precision VST_PREC_FP32: exact-fp32 MFMA (one sweep per slot present in a pixel group); otherwise,
 *                         when L % 64 == 0, bf16 MFMA with split operands (~1.5e-5): HBM-bound however the labels are mixed.
 * max_slots (1..32, 0 = 32) bounds the slots the launches cover when the host knows it (e.g. a plan reused over a clip);
 * nothing here synchronises with the host. */
#define VST_LABEL_PLAN_BYTES 2344
int vst_label_plan(const uint8_t* cmask, long Lc, const uint8_t* smask, long Ls, void* plan, void* stream);
size_t vst_cwct_labels_workspace_bytes(int N, long L);
int vst_cwct_stats_labels(const float* x, int N, long L, const uint8_t* mask, const void* plan, int max_slots,
                          double* stats, void* workspace, void* stream);
int vst_cwct_factor_labels(const double* content_stats, const double* style_stats, const void* plan, int max_slots,
                           float eps, int N, float* affines, int* info, void* stream);
int vst_cwct_apply_labels(const float* x, float* y, int N, long L, const float* affines, const uint8_t* mask,
                          const void* plan, int max_slots, int precision, void* stream);

/* ---- mask producers (csrc/masks.hip): what a label map needs before the masked transfer, on the device --------------------
 * For a clip with one label map per frame (video_transfer.py:161-186 of the reference: change_seg, self_remapping,
 * cross_remapping, then transfer with that frame's content_seg).  Stream-ordered, nothing allocated, nothing synchronised.
 * vst_colors_to_labels : utils/utils.py:104-137 (change_seg): uint8 RGB [n][3] -> uint8 labels with the nine-colour
 *                        dictionary: smallest L1 distance (0 for an exact match), ties keep the earlier dictionary entry.
 * vst_label_hist       : hist = int[256] (overwritten) of a uint8 label map.
 * vst_mask_prepare     : the one pass over an uploaded map: src = uint8 [H][W][3] colours (colours != 0) or uint8 [H][W]
 *                        labels (4-byte aligned); writes the labels in the packed code's row order (vst_mask_to_code's
 *                        mapping) and their histogram (int[256], overwritten).
 * vst_remap_lut        : models/segmentation/SegReMapping.py:19-76 as a 256-entry table.  table = int16 [rows][cols], column l
 *                        lists the labels most related to l, best first.  self_remapping when min_count > 0: a label with
 *                        0 < hist < min_count moves to the first related label with hist >= min_count (min_count = the
 *                        smallest count whose float32 share of the map reaches min_ratio, computed by the caller with the host
 *                        class's own expression).  cross_remapping when style_hist != NULL: a label of the (self-remapped)
 *                        map with style_hist == 0 moves to the first related label with style_hist > 0.  lut = cross o self
 *                        (identity for labels the map does not hold), hist_out = histogram of the remapped map (may be NULL).
 *                        A label that needs a lookup but is >= cols stays and ORs VST_MASK_OUT_OF_TABLE into *flags.
 * vst_apply_lut        : out[p] = lut[in[p]] (out may alias in).
 * vst_label_plan_hist  : vst_label_plan from histograms: hist_c of the RAW map, remap_lut (NULL = identity), hist_s of the
 *                        style map; at most max_slots (1..32) slots, more valid labels set plan.overflow and OR
 *                        VST_MASK_OVERFLOW into *flags (flags may be NULL).  plan.lut[raw] = slot of remap_lut[raw], slot_label
 *                        = the remapped label, hist_c = the remapped map's histogram: the statistics / apply / decode kernels
 *                        read plan.lut[mask[p]] with the RAW labels, the remapped map is never written.
 * vst_cwct_factor_labels_keyed : vst_cwct_factor_labels with the style statistics in the slot order of `style_plan` (a plan of
 *                        the style map against itself: every label with more than 10 style pixels has a slot): content slot k
 *                        pairs with the style slot whose slot_label equals plan.slot_label[k] - same arithmetic, same bits.  A
 *                        content slot without a style slot (more than 32 style labels) gets the identity map and info[slot][1] = 2.
 * ---- style interpolation under masks (cWCT.interpolation, models/cWCT.py:206-262, taken per label like _transfer_seg :49-109;
 *      the reference's scripts say "mask is not supported" there, video_transfer.py:198-201 / image_transfer.py:192-196) ----
 * vst_label_plan_hists : vst_label_plan_hist against n_styles (1..8) style histograms (host array of device pointers): a label
 *                        has a slot iff the rule of compute_label_info (cWCT.py:178) holds against EVERY style map; the same
 *                        plan record (hist_s = the smallest style count), slots in increasing label order, the same overflow
 *                        behaviour and max_slots cap.  With one style it is vst_label_plan_hist.
 * vst_cwct_factor_labels_mix : one workgroup per slot k: T_k = (sum_i alpha_i chol(Cs_i,k) [blended with chol(Cc,k) by alpha_c])
 *                        chol(Cc,k)^-1 and t0_k as vst_cwct_factor gives them (cWCT.py:228-262).  style_stats_host_array[i] =
 *                        double[32][1 + N + N*N] (raw or prefactored records); style_plans_host_array (may be NULL) [i] = the plan
 *                        style i's records are keyed by (as in vst_cwct_factor_labels_keyed), or NULL = the slot order of `plan`.
 *                        info = int[32][2 + n_styles] = {content retries, flag, style retries...}.  A slot whose label is missing
 *                        from any keyed style gets the identity map and flag 2.  One style, alpha 1, alpha_c 0: the bits of
 *                        vst_cwct_factor_labels / _keyed.
 * vst_cwct_prefactor_labels : vst_cwct_prefactor for every slot `plan` has of a double[32][1 + N + N*N] block (out may alias
 *                        stats; info = int[32] retries): a bound style then costs no Cholesky per frame.  The factor reads the
 *                        stored fp32 factor back exactly, so affines from prefactored and raw records are the same bits. */
#define VST_MASK_OVERFLOW 1u
#define VST_MASK_OUT_OF_TABLE 2u
int vst_colors_to_labels(const uint8_t* rgb, uint8_t* labels, long n, void* stream);
int vst_label_hist(const uint8_t* labels, long n, int* hist, void* stream);
int vst_mask_prepare(const uint8_t* src, int colours, int H, int W, uint8_t* mask_rows, int* hist, void* stream);
int vst_remap_lut(const int* hist, const int* style_hist, const int16_t* table, int rows, int cols, int min_count,
                  uint8_t* lut, int* hist_out, unsigned* flags, void* stream);
int vst_apply_lut(const uint8_t* in, const uint8_t* lut, uint8_t* out, long n, void* stream);
int vst_label_plan_hist(const int* hist_c, const uint8_t* remap_lut, const int* hist_s, int max_slots, void* plan,
                        unsigned* flags, void* stream);
int vst_cwct_factor_labels_keyed(const double* content_stats, const double* style_stats, const void* plan,
                                 const void* style_plan, int max_slots, float eps, int N, float* affines, int* info,
                                 void* stream);
int vst_label_plan_hists(const int* hist_c, const uint8_t* remap_lut, const int* const* hist_s_host_array, int n_styles,
                         int max_slots, void* plan, unsigned* flags, void* stream);
int vst_cwct_factor_labels_mix(const double* content_stats, const double* const* style_stats_host_array,
                               const void* const* style_plans_host_array, const float* alphas_host, int n_styles,
                               float alpha_c, const void* plan, int max_slots, float eps, int N, float* affines, int* info,
                               void* stream);
int vst_cwct_prefactor_labels(const double* stats, const void* plan, int max_slots, int N, float eps, double* out, int* info,
                              void* stream);

/* Turns a statistics record into a "prefactored" one ({-(n+1), mean, chol(cov) with jitter retries}); a style that
 * is reused over many frames (video_transfer.py re-factors it per frame, :195-203) then costs no Cholesky in
 * vst_cwct_factor.  `out` may alias `stats`; info = int[1] retry count. */
int vst_cwct_prefactor(const double* stats, int N, float eps, double* out, int* info, void* stream);

/* ---- generic-architecture RevResNet ops -------------------------------------------------------------------------------------
 * models/RevResNet.py:166-201 accepts any nBlocks / nStrides / nChannels / mult / kernel / in_channel / hidden_dim / sp_steps; the
 * whole-pass entry points above implement the published architecture ([10,10,10] / [1,2,2] / [16,64,256], mult 4, kernel 3).
 * Any other architecture runs on these: plain NCHW fp32 tensors, exact fp32 FMA (the slow, complete path; csrc/generic.hip).
 *   vst_generic_conv : ReflectionPad2d((K-1)/2) + Conv2d(K, stride, bias=True) of residual_block.conv (:79-88), K odd <= 7,
 *                      stride 1 or 2; relu != 0 applies ReLU; old != NULL: out = old + sign * conv (the coupling of
 *                      residual_block.forward / .inverse, :96-116; out may alias old).  w = OIHW, out = [B,Cout,Ho,Wo],
 *                      Ho = (H + 2 pad - K) / stride + 1.
 *   vst_generic_squeeze / _unsqueeze : :34-43 (D, H, W = channels and size of the UNsqueezed tensor, H, W even).
 *   vst_generic_copy_channels : dst[b, d0 + k] = src[b, c0 + k], k < n  (split / merge / injective_pad, :8-31); vst_generic_zero. */
int vst_generic_conv(const float* x, const float* w, const float* bias, const float* old, float sign, int relu, float* out, int B,
                     int Cin, int Cout, int H, int W, int K, int stride, void* stream);
int vst_generic_squeeze(const float* x, float* y, int B, int D, int H, int W, void* stream);
int vst_generic_unsqueeze(const float* y, float* x, int B, int D, int H, int W, void* stream);
int vst_generic_copy_channels(const float* src, float* dst, int B, int C_src, int c0, int n, long HW, int C_dst, int d0,
                              void* stream);
int vst_generic_zero(float* dst, size_t n_floats, void* stream);

/* ---- fp64 cWCT: cWCT(use_double=True), models/cWCT.py:13-16,35-47,66,106,220,238,259 -------------------------------------
 * The reference converts the features to double and runs mean / covariance / Cholesky (with the same jitter schedule) / inverse
 * / both products in fp64, then converts back.  Same records as the fp32 calls (stats = double[1 + N + N*N], info as in
 * vst_cwct_factor) but: true fp64 two-pass statistics, an fp64 factorisation, affine = DOUBLE[N*N + N], and the apply
 * accumulates in fp64 (y = float(T double(x) + t0); y may alias x; with a mask only matching pixels are written).
 * A fidelity option, not a hot path (no script of the reference sets it): NCHW codes only, N in {16, 32, 64, 128}.
 * workspace: 256-byte aligned, as every allocator here returns it. */
size_t vst_cwct_stats_f64_workspace_bytes(int N, long L);
int vst_cwct_stats_f64(const float* x, int N, long L, const uint8_t* mask, int label, double* stats, void* workspace,
                       void* stream);
size_t vst_cwct_factor_f64_workspace_bytes(int N);
int vst_cwct_factor_f64(const double* content_stats, const double* const* style_stats_host_array, const float* alphas_host,
                        int n_styles, float alpha_c, float eps, int N, double* affine, int* info, void* workspace,
                        void* stream);
int vst_cwct_apply_f64(const float* x, float* y, int N, long L, const double* affine, const uint8_t* mask, int label,
                       void* stream);

/* ---- any code width: cWCT for N = 1..256 (csrc/cwct_any.hip) ------------------------------------------------------------------
 * models/cWCT.py:111-262 (cholesky_dec, whitening, coloring, _transfer_seg, interpolation) for every N; a RevResNet with another
 * hidden_dim (models/RevResNet.py:166-201) has a code of N = 2 * hidden_dim channels.  The calls above keep their contract
 * (N in {16, 32, 64, 128}, VST_E_SHAPE otherwise); these take any 1 <= N <= 256 and return VST_E_SHAPE outside it, VST_E_ARG for
 * a null pointer or n_styles outside 1..8, VST_E_WORKSPACE for a null workspace or one of fewer than the *_workspace_bytes bytes
 * (`workspace_bytes` = the caller's size).  Checks run before any launch.
 *   vst_cwct_stats_n     : vst_cwct_stats (same {n, mean, cov} record, same mask / label selection, fp32 shifted per-workgroup
 *                          sums combined in fp64).
 *   vst_cwct_factor_n    : vst_cwct_factor (same affine record float[N*N + N], info IN/OUT, prefactored records accepted);
 *                          the factorisation runs in `workspace`.
 *   vst_cwct_prefactor_n : vst_cwct_prefactor (out may alias stats; workspace of vst_cwct_factor_n_workspace_bytes).
 *   vst_cwct_apply_n     : y[:,p] = T x[:,p] + t0 in exact fp32 (y may alias x; with a mask only matching pixels are written).
 *   *_f64                : the fp64 calls (vst_cwct_stats_f64 / factor_f64 / apply_f64) at these widths.
 * workspace: 256-byte aligned, as every allocator here returns it. */
size_t vst_cwct_stats_n_workspace_bytes(int N, long L);
int vst_cwct_stats_n(const float* x, int N, long L, const uint8_t* mask, int label, double* stats, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t vst_cwct_factor_n_workspace_bytes(int N);
int vst_cwct_factor_n(const double* content_stats, const double* const* style_stats_host_array, const float* alphas_host,
                      int n_styles, float alpha_c, float eps, int N, float* affine, int* info, void* workspace,
                      size_t workspace_bytes, void* stream);
int vst_cwct_prefactor_n(const double* stats, int N, float eps, double* out, int* info, void* workspace, size_t workspace_bytes,
                         void* stream);
int vst_cwct_apply_n(const float* x, float* y, int N, long L, const float* affine, const uint8_t* mask, int label, void* stream);
size_t vst_cwct_stats_n_f64_workspace_bytes(int N, long L);
int vst_cwct_stats_n_f64(const float* x, int N, long L, const uint8_t* mask, int label, double* stats, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t vst_cwct_factor_n_f64_workspace_bytes(int N);
int vst_cwct_factor_n_f64(const double* content_stats, const double* const* style_stats_host_array, const float* alphas_host,
                          int n_styles, float alpha_c, float eps, int N, double* affine, int* info, void* workspace,
                          size_t workspace_bytes, void* stream);
int vst_cwct_apply_n_f64(const float* x, float* y, int N, long L, const double* affine, const uint8_t* mask, int label,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement hook (bench.py's live roofline figure): bracket every launch of one conv kernel class
 * with HIP events on the launch stream.  One profiling session at a time (begin/end and the launch
 * sites are serialised by a lock, so other host threads may keep launching while a session runs).
 *   vst_profile_begin(VST_KERNEL_ID(cin,cout,stride), max_records); ...run passes...;
 *   vst_profile_end(&total_ms, &launches)   (synchronises on the recorded events)
 * ------------------------------------------------------------------------------------------- */
#define VST_KERNEL_ID(cin, cout, stride) (((cin) << 16) | ((cout) << 4) | (stride))
#define VST_KERNEL_ALL (-1)        /* every hooked launch; read the session with vst_profile_end_table */
/* ids of the non-conv launches (one per C entry point) */
#define VST_KERNEL_PACK 1          /* vst_pack_input* (+ the folded block-0 constant) */
#define VST_KERNEL_UNPACK 2
#define VST_KERNEL_SPREAD 3
#define VST_KERNEL_GATHER 4
#define VST_KERNEL_CWCT_STATS 5
#define VST_KERNEL_CWCT_FACTOR 6
#define VST_KERNEL_CWCT_APPLY 7
#define VST_KERNEL_PRESPLIT 8      /* fp32 state -> split fp16 planes in front of the first 256-channel block (F16X2) */
#define VST_KERNEL_SEG_MIX 9       /* vst_seg_mix_logits */
#define VST_KERNEL_CWCT_POOL 10     /* vst_cwct_stats_pool, vst_cwct_stats_pool_keyed */
int vst_profile_begin(int kernel_id, int max_records);
int vst_profile_end(double* total_ms, int* launches);
/* per-id totals of a VST_KERNEL_ALL (or single-id) session: ids[i], ms[i], launches[i] for i < *n_ids <= cap */
int vst_profile_end_table(int* ids, double* ms, int* launches, int cap, int* n_ids);

/* ---------------------------------------------------------------------------------------------
 * Process-wide tuning options (atomic; may be set at any time, a launch reads them when it is enqueued).
 *   VST_OPT_STAGE3_LEAN  1: the 256-channel convs of VST_PREC_BF16X3 (residual_block.conv of models/RevResNet.py:79-88 at
 *                        C = 256) run as half-CU workgroups (4 waves, 8 x 16 pixel tiles, 96 KB of LDS, <= 256 VGPRs) so that
 *                        an HBM-bound 16- / 64-channel workgroup (<= 61 KB of LDS) of ANOTHER frame on another stream shares the
 *                        CU - two lean workgroups (2 x 96 KB) do not fit one CU's 160 KB - for callers that keep several frames in
 *                        flight (video_transfer.py:160-214's loop run on HIP streams); 0: one workgroup per CU on 16 x 16 tiles,
 *                        in the form VST_OPT_STAGE3_WIDE selects.  Takes precedence over VST_OPT_STAGE3_WIDE.  Results are
 *                        bit-identical.  Initial value: environment variable VST_LEAN (0 / 1), else 0.
 *   VST_OPT_STAGE3_WIDE  1: those convs run as 4 waves (one per SIMD) that each own 4 rows of the 16 x 16 tile (a 64-channel x
 *                        64-pixel register tile, 512 registers per lane); 0: 8 waves (two per SIMD) that own 2 rows each.  Results
 *                        are bit-identical.  Initial value: environment variable VST_WIDE (0 / 1), else 1.
 *   VST_OPT_STAGE3_PINGPONG  reserved id of a removed experiment: both calls return VST_E_ARG for it.
 *   VST_OPT_STAGE1_FOLD  1: conv.1 (16 -> 4 channels) of the 16-channel blocks of VST_PREC_BF16X3 folds the horizontal tap into the
 *                        weight operand's rows (12 of 16 instead of 4) and adds the three shifted partial sums afterwards: half the
 *                        MFMAs; 0: the tap in K like every other conv.  The same products summed in another order (not
 *                        bit-identical, inside the mode's tolerance).  Initial value: VST_FOLD16 (0 / 1), else 1.
 *   VST_OPT_OUT_RGB      1: the last block of an inverse pass / decode in an MFMA mode writes the image (float NCHW or uint8 HWC)
 *                        from its conv.7 epilogue; 0: it updates the state and vst_unpack_output[_u8] runs as a launch of its own.
 *                        Results are bit-identical.  Initial value: VST_OUT_RGB (0 / 1), else 1.
 * vst_set_option returns VST_E_ARG for an unknown option, vst_get_option the value (or VST_E_ARG).
 * ------------------------------------------------------------------------------------------- */
#define VST_OPT_STAGE3_LEAN 1
#define VST_OPT_STAGE3_PINGPONG 2
#define VST_OPT_STAGE3_WIDE 3
#define VST_OPT_STAGE1_FOLD 4
#define VST_OPT_OUT_RGB 5
int vst_set_option(int option, int value);
int vst_get_option(int option);

/* ---------------------------------------------------------------------------------------------
 * Frame resampling around the stylisation (csrc/resize.hip): the two bicubic resizes utils/utils.py:90-101 (img_resize) applies
 * to every frame before the encoder (video_transfer.py:161), and the float resize to the writer size after the decoder
 * (video_transfer.py:210-212).  Both are separable: a horizontal pass into `tmp`, then a vertical pass.
 *
 * A TABLE for one axis (in_size -> out_size) is out_size * (2 + ksize) 32-bit words: bounds = int[out_size][2] = {first input
 * index, number of taps} followed by the coefficients [out_size][ksize] (taps past a row's count are 0).  ksize depends on the
 * sizes alone: 2 * ceil(2 * max(1, in/out)) + 1.
 *
 * vst_resize_coeffs_u8  : host only.  Pillow's 8-bit bicubic table (a = -0.5, support 2 * max(1, in/out), coefficients built
 *                        in double, normalised by their sum, rounded to 22-bit fixed point: (int)(+-0.5 + k * 2^22)), integer
 *                        for integer.  *ksize is always written; with bounds == NULL or kk == NULL nothing else is (size query).
 * vst_resize_u8         : one Image.resize((Wd, Hd), BICUBIC) of an RGB uint8 [Hs][Ws][3] frame, bit-exact: every pass computes
 *                        clip8((2^21 + sum px * k) >> 22) in int32; the horizontal pass comes first and its result is ROUNDED
 *                        TO UINT8 in tmp (uint8 [Hs][Wd][3]); a pass whose size does not change is skipped, equal sizes copy.
 *                        tables_dev = the horizontal table (Ws -> Wd; absent when Ws == Wd) followed by the vertical table
 *                        (Hs -> Hd; absent when Hs == Hd), on the device.  tmp may be NULL when at most one pass runs.
 * vst_resize_coeffs_u8_bilinear : host only.  Pillow's 8-bit table of Image.BILINEAR (the triangle filter, support max(1, in/out)):
 *                        the same normalisation, 22-bit rounding and bounds rule; ksize = 2 * ceil(max(1, in/out)) + 1.
 * vst_resize_grey_u8    : one Image.resize((Wd, Hd), BILINEAR) of an "L" image, uint8 [Hs][Ws] -> [Hd][Wd], bit-exact: the passes
 *                        of vst_resize_u8 on one channel (tmp = uint8 [Hs][Wd]) with the bilinear tables in tables_dev, laid out
 *                        as there.  A frame's matte takes it to the stylised size (vst_strength_frame).  Same limits and errors.
 * vst_resize_coeffs_f32 : host only.  The antialiased bicubic weights of F.interpolate(mode="bicubic", align_corners=False,
 *                        antialias=True): scale = in/out, support = 2 * max(scale, 1), center = scale * (i + 0.5), window
 *                        [max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in)), weights
 *                        cubic((j + xmin - center + 0.5) / max(scale, 1)) normalised; built in double, stored as fp32.
 *                        xmin = int[out][2] (the table's bounds), w = float[out][ksize]; NULL outputs: size query as above.
 * vst_resize_f32        : x = float [B][3][Hs][Ws] -> dst = float [B][3][Hd][Wd], fp32 accumulation (fma), horizontal pass
 *                        first into tmp = float [B][3][Hs][Wd] (not used, may be NULL, when Ws == Wd).  tables_dev = horizontal
 *                        table (absent when Ws == Wd) followed by the vertical table (always present).
 * vst_resize_f32_to_u8  : the same values, then * 255, clamp to [0, 255], truncate: uint8 [B][Hd][Wd][3].
 *
 * Limits: sizes are any positive integers (no multiple-of-4 rule); source, destination and the intermediate [Hs][Wd] are each
 * at most VST_MAX_FRAME_PIXELS pixels per image and a shrink factor is at most VST_RESIZE_MAX_SHRINK in either axis (ksize <=
 * 65), VST_E_SHAPE otherwise; VST_E_ARG for a null pointer or a non-positive size.  All checks come before any launch.
 * ------------------------------------------------------------------------------------------- */
#define VST_RESIZE_MAX_SHRINK 16
int vst_resize_coeffs_u8(int in_size, int out_size, int* ksize, int* bounds, int* kk);
int vst_resize_u8(const uint8_t* src_hwc, int Hs, int Ws, uint8_t* dst_hwc, int Hd, int Wd, const int* tables_dev,
                  uint8_t* tmp, void* stream);
int vst_resize_coeffs_u8_bilinear(int in_size, int out_size, int* ksize, int* bounds, int* kk);
int vst_resize_grey_u8(const uint8_t* src, int Hs, int Ws, uint8_t* dst, int Hd, int Wd, const int* tables_dev, uint8_t* tmp,
                       void* stream);
int vst_resize_coeffs_f32(int in_size, int out_size, int* ksize, int* xmin, float* w);
int vst_resize_f32(const float* x_planar, int B, int Hs, int Ws, float* dst_planar, int Hd, int Wd, const void* tables_dev,
                   float* tmp, void* stream);
int vst_resize_f32_to_u8(const float* x_planar, int B, int Hs, int Ws, uint8_t* dst_hwc, int Hd, int Wd,
                         const void* tables_dev, float* tmp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * On-device segmentation (csrc/segformer.hip): SegmentModel of project/image_style/segment.py:471-532 - the MiT backbone
 * (VisionTransformer, :137-267) and SegFormerHead (:391-468) - from a uint8 frame to a uint8 ADE20K label map.
 *
 * A PLAN holds one network's weights on the device it was created on, and one workspace per stream it has run on.  These are
 * the library's only device allocations: vst_seg_create allocates the weights, a run allocates (or grows) its stream's
 * workspace the first time it sees a frame size; after that a run is stream-ordered launches with no host synchronisation.
 * Runs on different streams do not share scratch memory.
 *
 * vst_seg_create      : depths[4] = blocks per stage (B1 {2,2,2,2}, B2 {3,4,6,3}, B3 {3,4,18,3}, B4 {3,8,27,3}, B5 {3,6,40,3});
 *                       embed_dim = the decode head's width (768; 256 for B1), a multiple of 4.  embed_dims {64,128,320,512},
 *                       heads {1,2,5,8} and sr_ratios {8,4,2,1} are fixed.
 * vst_seg_tensor_count / vst_seg_tensor_info : the tensors the plan needs, in order: name and element count.
 * vst_seg_load_tensor : copies `count` floats from HOST memory (synchronous; load time only).  VST_E_ARG for an unknown name,
 *                       VST_E_SHAPE for a wrong count.  Names are the reference's state-dict keys under backbone.*, except:
 *                         - conv weights are [out][ky][kx][in] (the patch gather's K order): patch_embed{1..4}.proj.weight,
 *                           block*.attn.sr.weight;
 *                         - mlp.dwconv.dwconv.weight is [9][C] (tap-major);
 *                         - the decode head arrives FOLDED (vstnet_amd/segformer.py, fold_decode_head, in fp64):
 *                           decode_head.fold_c{1..4}.weight [E][C_i] = bn_scale * W_fuse[:, slice_i] * W_linear_ci,
 *                           decode_head.fold.bias [E] (the four linear biases through W_fuse, and the BatchNorm shift),
 *                           decode_head.linear_pred.weight [150][E], decode_head.linear_pred.bias [150].
 * vst_seg_run_u8      : frame_u8 = uint8 [H][W][3] (chw = 0) or [3][H][W] (chw = 1), any H, W >= 32 with
 *                       H * W <= 2^24 (VST_E_SHAPE otherwise: there is no tiled segmentation); labels_u8 = uint8 [H][W].
 *                       VST_E_ARG if a tensor was never loaded or the current device is not the plan's.
 * vst_seg_run_scaled_u8 : the same network on a WORKING frame, labels at another size ("Working resolution").
 *                       work_u8 = uint8 [Hw][Ww][3] or [3][Hw][Ww] under vst_seg_run_u8's rules (Hw, Ww >= 32,
 *                       Hw * Ww <= 2^24) - normally the PIL-exact bicubic downscale of an H x W frame (vst_resize_u8);
 *                       labels_u8 = uint8 [H][W] with H * W <= VST_SEG_MAX_LABEL_PIXELS:
 *                           labels = argmax_c F.interpolate(logits_q, size=(H, W), mode="bilinear", align_corners=False)
 *                       in ONE bilinear step from the padded working frame's quarter-resolution logits (ties to the lowest
 *                       class).  VST_E_SHAPE for either size, before any launch.  vst_seg_run_u8(H, W) is this call with
 *                       (Hw, Ww) = (H, W).  A second sampler, which stages each output tile's logit cells in LDS
 *                       and returns the per-pixel sampler's labels bit for bit, is dispatched from a measured upsampling
 *                       factor on (DESIGN.md has the threshold; until it is measured no run takes it).
 * vst_seg_labels_from_logits : for tests.  The sampling + argmax step alone, from logits = float [Hq*Wq][150] (8-byte aligned,
 *                       Hq * Wq <= 2^20) to labels uint8 [H][W]; kernel 0 = the per-pixel sampler, 1 = the tiled one
 *                       (VST_E_SHAPE where its tile does not fit LDS: factors under 4), -1 = the dispatch of a run.
 * vst_seg_logits      : for tests.  logits = float [Hq*Wq][150] at the padded frame's quarter resolution, token-major; x1..x4
 *                       (each may be NULL) = the four stage outputs, token-major [h_i*w_i][C_i].
 * vst_seg_shape       : host only.  hw8 = {h1, w1, h2, w2, h3, w3, h4, w4}, the four stage grids of an H x W frame.
 * vst_seg_mix_logits  : the temporal window of the video loop ("Temporal window"): out[i] = sum_k w[k] * x_k[i] over
 *                       the logits of n = 1..VST_SEG_MIX_MAX frames, one elementwise launch.  logits_host_array[k] = the DEVICE
 *                       pointer of the logits of age k (k = 0: the current frame), weights_host[k] = its fp32 weight; both
 *                       arrays live on the HOST and travel by value in the kernel arguments (no device-side table, no copy).
 *                       count = Hq * Wq * 150 floats: even, at most 2^20 * 150.  Every pointer is 8-byte aligned (what
 *                       vst_seg_labels_from_logits asks of its input); out overlaps none of the inputs (inputs may repeat).
 *                       Arithmetic: acc = w[0] * x_0; acc = acc + w[1] * x_1; ... in increasing age, every product and every
 *                       sum rounded to fp32, no fused multiply-add: n = 1 with w[0] = 1 copies the bits.  Bilinear sampling is
 *                       linear, so vst_seg_labels_from_logits of `out` gives the labels of the window's mean sampled logits.
 *                       VST_E_ARG: a null or misaligned pointer, out overlapping an input; VST_E_SHAPE: n outside
 *                       1..VST_SEG_MIX_MAX, count 0, odd or over the limit.  Nothing is launched on an error.  The launch is
 *                       profiled as VST_KERNEL_SEG_MIX.
 *
 * KERNEL-LEVEL CALLS, for tests and tools (tests/test_gpu_segformer_ops.py): one per kernel of the network, each the argument
 * checks below and then the launch helper a run uses, so the launch geometry is the production one.  Stream-ordered, nothing
 * allocated.  Maps are token-major fp32 [tokens][C].  VST_E_ARG: a null pointer (where NULL is not allowed), a float pointer
 * off the 16-byte grid; VST_E_SHAPE: the conditions named per call, a non-positive size, an operand of more than 2^30 floats.
 * Every refusal comes before any launch.
 * vst_seg_gemm        : out[M][N] = A[M][K] . W[N][K]^T (+ bias[N]) (+ res[M][N]); bias, res may be NULL, res may be out.
 *                       Six bf16 MFMA products of the three-way split operands, fp32 accumulation.  Any M, N, K >= 1.
 * vst_seg_layernorm   : out[T][C] = LayerNorm(x) * g + b over C, 1 <= C <= 512; out may be x.
 * vst_seg_attention   : out[N][C] = softmax(q k^T scale) v per head of 64 channels: q [N][C], kv [Nk][2C] with K of head h at
 *                       column 64 h and V at C + 64 h; C a multiple of 64, at most 512; N, Nk >= 1.
 * vst_seg_dwconv_gelu : out = GELU(depthwise 3x3 conv (zero padding) + b) of the H x W map in [H*W][C]; w [9][C]; C % 4 == 0.
 * vst_seg_im2col      : in [Hi*Wi][C] -> col [Ho*Wo][k*k*C] (K order ky, kx, c) of a k x k conv of the given stride and zero
 *                       padding, Ho = (Hi + 2 pad - k) / stride + 1 and Wo alike; C % 4 == 0, 1 <= k <= 64, 0 <= pad < k.
 * vst_seg_gather_rgb  : the frame of vst_seg_run_u8 -> col [h1*w1][147], the rows of patch_embed1's GEMM (replicate padding
 *                       to multiples of 4, / 255, ImageNet mean / std, then the 7 x 7 stride-4 conv's zero padding);
 *                       H, W as vst_seg_shape takes them.
 * vst_seg_head_sum    : out[h1*w1][E] = ReLU(y0 + up(y1) + up(y2) + up(y3)), up = bilinear to y0's grid (align_corners =
 *                       False); y_i [h_i*w_i][E], hw8 = the HOST array vst_seg_shape fills; E % 4 == 0; out may be y0.
 * ------------------------------------------------------------------------------------------- */
#define VST_SEG_CLASSES 150
#define VST_SEG_MAX_LABEL_PIXELS (1LL << 30)
#define VST_SEG_MIX_MAX 8
typedef struct vst_seg vst_seg;
int vst_seg_create(const int* depths, int embed_dim, vst_seg** plan);
int vst_seg_tensor_count(const vst_seg* plan);
int vst_seg_tensor_info(const vst_seg* plan, int index, const char** name, size_t* count);
int vst_seg_load_tensor(vst_seg* plan, const char* name, const float* data_host, size_t count);
int vst_seg_run_u8(vst_seg* plan, const uint8_t* frame_u8, int chw, int H, int W, uint8_t* labels_u8, void* stream);
int vst_seg_run_scaled_u8(vst_seg* plan, const uint8_t* work_u8, int chw, int Hw, int Ww, int H, int W, uint8_t* labels_u8,
                          void* stream);
int vst_seg_labels_from_logits(const float* logits, int Hq, int Wq, int H, int W, int kernel, uint8_t* labels, void* stream);
int vst_seg_logits(vst_seg* plan, const uint8_t* frame_u8, int chw, int H, int W, float* logits, float* x1, float* x2,
                   float* x3, float* x4, void* stream);
int vst_seg_shape(int H, int W, int* hw8);
int vst_seg_mix_logits(const float* const* logits_host_array, const float* weights_host, int n, size_t count, float* out,
                       void* stream);
int vst_seg_destroy(vst_seg* plan);
/* kernel-level calls (tests and tools) */
int vst_seg_gemm(const float* A, const float* W, const float* bias, const float* res, float* out, int M, int N, int K,
                 void* stream);
int vst_seg_layernorm(const float* x, const float* g, const float* b, float* out, int T, int C, float eps, void* stream);
int vst_seg_attention(const float* q, const float* kv, float* out, int N, int Nk, int C, float scale, void* stream);
int vst_seg_dwconv_gelu(const float* in, const float* w, const float* b, float* out, int H, int W, int C, void* stream);
int vst_seg_im2col(const float* in, int Hi, int Wi, int C, int k, int stride, int pad, float* col, void* stream);
int vst_seg_gather_rgb(const uint8_t* frame_u8, int chw, int H, int W, float* col, void* stream);
int vst_seg_head_sum(const float* y0, const float* y1, const float* y2, const float* y3, const int* hw8, int E, float* out,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Style loss (csrc/vgg.hip; DESIGN.md section 6, "Style loss"): the reference's VGG-19 encoder up to relu4_1 (models/VGG.py,
 * build_vgg, Sequential indices 0 .. 29: a 1 x 1 conv 3 -> 3, nine 3 x 3 convs under ReflectionPad2d(1) with ReLU, three
 * 2 x 2 / stride-2 max-pools with ceil_mode behind relu1_2, relu2_2, relu3_4), the mean / std records of its taps relu1_1,
 * relu2_1, relu3_1, relu4_1 and the reference's loss_s and loss_c from them.  Maps are token-major fp32 [H*W][C].
 *
 * A PLAN holds the encoder's weights on the device it was created on (the only device allocation here; a run works in the
 * caller's workspace and is stream-ordered launches with no host synchronisation).
 * vst_vgg_create / vst_vgg_destroy.
 * vst_vgg_load_tensor : copies `count` floats from HOST memory (synchronous; load time only).  Names and shapes are the
 *                       reference checkpoint's: "<index>.weight" [Cout][Cin][3][3] ([3][3][1][1] for index 0), "<index>.bias"
 *                       [Cout], index in {0, 2, 5, 9, 12, 16, 19, 22, 25, 29}.  A 3 x 3 weight is repacked to [Cout][9 Cin] in K
 *                       order (ky, kx, c), the first one padded from 3 to 4 input channels with zeros.  VST_E_ARG for an unknown
 *                       name (the layers past relu4_1 are not taken), VST_E_SHAPE for a wrong count.
 * vst_vgg_workspace_bytes : host only.  The bytes a features run on an H x W frame needs at `ws` (16-byte aligned): the
 *                       [H*W][4] input map, two maps of H W 64 floats and the reductions' partial sums.
 * vst_vgg_features_u8 / _f32 : frame = uint8 [H][W][3] or float [3][H][W] -> records = double[VST_VGG_RECORD_DOUBLES]: per tap
 *                       [2][C_l] (means, then stds), C = 64, 128, 256, 512, one after the other; relu4_1 (may be NULL) =
 *                       float [h4*w4][512] with h_{l+1} = ceil(h_l / 2), 16-byte aligned.  VST_E_SHAPE if a level's edge
 *                       would be under 2 (H or W under 9) or H * W > 2^24; VST_E_WORKSPACE for a null or misaligned ws
 *                       or fewer than vst_vgg_workspace_bytes bytes; VST_E_ARG for a null or misaligned pointer, a null plan, a tensor never loaded, or
 *                       another current device than the plan's.  Every refusal comes before any launch.
 *
 * KERNEL-LEVEL CALLS (tests/test_gpu_vgg_ops.py): each the argument checks below and then the launch helper a run uses.
 * Stream-ordered, nothing allocated.  VST_E_ARG: a null pointer, a map or weight pointer off the 16-byte grid, a double pointer
 * off the 8-byte grid, overlapping in / out; VST_E_SHAPE: the conditions named per call, a non-positive size, an operand of
 * more than 2^30 floats, a map of more than 2^24 pixels.  Every refusal comes before any launch.
 * vst_vgg_input_u8    : out[H*W][4] from a uint8 [H][W][3] frame: x = v / 255 in fp32, then the 1 x 1 conv w9 = A[3][3], b3 (device
 *                       pointers), y_o = ((A_o0 x0 + A_o1 x1) + A_o2 x2) + b_o with every product and sum rounded to fp32;
 *                       channel 3 is 0.  Any H, W >= 1.  vst_vgg_input_f32: the same from float [3][H][W] (x = v).
 * vst_vgg_conv3x3_relu : out[H*W][Cout] = ReLU(conv3x3(reflect_pad1(in[H*W][Cin])) + bias), w = [Cout][9 Cin] in K order (ky, kx,
 *                       c).  An implicit GEMM: vst_seg_gemm's kernel with a gathering A-loader, so the result is
 *                       ReLU(vst_seg_gemm(col, w, bias)) bit for bit, col the [H*W][9 Cin] reflect-gathered column matrix, which
 *                       is never formed.  Cin % 4 == 0, Cin >= 4, Cout >= 1, H, W >= 2.  out may not overlap in.
 * vst_vgg_maxpool2    : [H*W][C] -> [ceil(H/2) ceil(W/2)][C], partial windows at odd edges (ceil_mode); C % 4 == 0, H, W >= 1.
 * vst_vgg_mean_std    : out = double [2][C]: per channel over the n rows of in[n][C], in fp64, two passes: the mean, then
 *                       sqrt(sum (x - mean)^2 / (n - 1) + eps).  A fixed reduction order, no atomics.  n >= 2.  ws = at least
 *                       vst_vgg_mean_std_workspace_bytes(n, C) bytes on an 8-byte address (VST_E_WORKSPACE otherwise).
 * vst_vgg_mse_f64     : out[0] = mean (a_i - b_i)^2 over `count` floats, in fp64, a fixed order; ws = VST_VGG_MSE_WS_BYTES bytes.
 *                       workspace: 256-byte aligned, as every allocator here returns it.
 * vst_vgg_style_loss  : out[0] = sum_l mse(mean_a, mean_b) + mse(std_a, std_b) from two record sets as vst_vgg_features writes.
 * ------------------------------------------------------------------------------------------- */
#define VST_VGG_RECORD_DOUBLES 1920
#define VST_VGG_MSE_WS_BYTES 8192
typedef struct vst_vgg vst_vgg;
int vst_vgg_create(vst_vgg** plan);
int vst_vgg_load_tensor(vst_vgg* plan, const char* name, const float* data_host, size_t count);
int vst_vgg_workspace_bytes(int H, int W, size_t* bytes);
int vst_vgg_features_u8(vst_vgg* plan, const uint8_t* frame_hwc_u8, int H, int W, double* records, float* relu4_1, void* ws,
                        size_t ws_bytes, void* stream);
int vst_vgg_features_f32(vst_vgg* plan, const float* frame_planar, int H, int W, double* records, float* relu4_1, void* ws,
                         size_t ws_bytes, void* stream);
int vst_vgg_destroy(vst_vgg* plan);
/* kernel-level calls (tests and tools) */
int vst_vgg_input_u8(const uint8_t* frame_hwc_u8, const float* w9, const float* b3, float* out, int H, int W, void* stream);
int vst_vgg_input_f32(const float* frame_planar, const float* w9, const float* b3, float* out, int H, int W, void* stream);
int vst_vgg_conv3x3_relu(const float* in, const float* w, const float* bias, float* out, int H, int W, int Cin, int Cout,
                         void* stream);
int vst_vgg_maxpool2(const float* in, float* out, int H, int W, int C, void* stream);
int vst_vgg_mean_std_workspace_bytes(int n, int C, size_t* bytes);
int vst_vgg_mean_std(const float* in, int n, int C, double eps, double* out, void* ws, size_t ws_bytes, void* stream);
int vst_vgg_mse_f64(const float* a, const float* b, size_t count, double* out, void* ws, void* stream);
int vst_vgg_style_loss(const double* records_a, const double* records_b, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Raw video edge ("Raw video edge"): 8-bit Y'CbCr planes <-> the uint8 HWC RGB frame of the video loop, so
 * that a YUV4MPEG2 frame goes up and comes back as its 1.5 bytes per pixel.  Planes are dense: y[H][W]; u, v [H][W] (VST_YUV_444)
 * or [(H+1)/2][(W+1)/2] (4:2:0).  Any H, W >= 1 with H * W <= VST_MAX_FRAME_PIXELS.
 *   layout  VST_YUV_444; VST_YUV_420_CENTRE (y4m C420jpeg, C420): chroma sample (i, j) sits at luma (2i + 1/2, 2j + 1/2);
 *           VST_YUV_420_LEFT (C420mpeg2): horizontally on the even luma columns, vertically centred.
 *   matrix  VST_YUV_BT601 (Kr 0.299, Kb 0.114), VST_YUV_BT709 (Kr 0.2126, Kb 0.0722); Kg = 1 - Kr - Kb.
 *   range   VST_YUV_LIMITED: Y offset 16, scale 219, chroma scale 224; VST_YUV_FULL: 0, 255, 255.  Chroma offset 128 in both.
 * vst_yuv_to_rgb_u8: y' = (Y - yoff) 255 / ys, pb = (U - 128) 255 / cs, pr = (V - 128) 255 / cs; R = y' + 2 (1 - Kr) pr,
 *   B = y' + 2 (1 - Kb) pb, G = y' - (2 (1 - Kr) Kr / Kg) pr - (2 (1 - Kb) Kb / Kg) pb; a byte is clamp(floor(v + 0.5), 0, 255).
 *   4:2:0: U and V are sampled bilinearly at the siting - the chroma coordinate of luma x is (x - 1/2) / 2 (centre) or x / 2
 *   (left), of luma y always (y - 1/2) / 2; neighbour indices are clamped to the plane - on the raw bytes, in float, before the
 *   matrix: one rounding, at the end.
 * vst_rgb_to_yuv_u8: Y = Kr R + Kg G + Kb B, Cb = (B - Y) / (2 (1 - Kb)), Cr = (R - Y) / (2 (1 - Kr)) on 0..255 values; bytes
 *   clamp(floor(yoff + Y ys / 255 + 0.5)) and clamp(floor(128 + C cs / 255 + 0.5)).  4:2:0: the float Cb, Cr are averaged before
 *   that one rounding - over the two rows, and over the two columns (centre) or with [1/4, 1/2, 1/4] around the even column
 *   (left); a missing neighbour (odd H, odd W, the frame border) is the edge pixel again.
 * fp32 arithmetic: a byte equals floor(v + 0.5) of the exact value v unless v lies within 2^-10 of a tie (tests/yuv_ref.py).
 * VST_E_ARG for a null pointer, an unknown layout / matrix / range, H or W < 1 or H * W past VST_MAX_FRAME_PIXELS; checks come
 * before any launch.  Pointers need no alignment (aligned ones take the dword paths). */
#define VST_YUV_444 0
#define VST_YUV_420_CENTRE 1
#define VST_YUV_420_LEFT 2
#define VST_YUV_BT601 0
#define VST_YUV_BT709 1
#define VST_YUV_LIMITED 0
#define VST_YUV_FULL 1
int vst_yuv_to_rgb_u8(const uint8_t* y, const uint8_t* u, const uint8_t* v, int H, int W, int layout, int matrix, int range,
                      uint8_t* rgb_hwc, void* stream);
int vst_rgb_to_yuv_u8(const uint8_t* rgb_hwc, int H, int W, int layout, int matrix, int range, uint8_t* y, uint8_t* u,
                      uint8_t* v, void* stream);

/* ---------------------------------------------------------------------------------------------
 * High-bit-depth edge ("High-bit-depth edge"): 9..16-bit Y'CbCr planes <-> fp32 RGB planes [3][H][W] on a
 * 0..1 scale, so that a frame of headerless raw YUV (yuv420p10le, yuv422p10le, ...) enters the encoder and leaves the decoder
 * without passing through 256 levels.  Samples are little-endian 16-bit in dense planes: y[H][W]; u, v [H][W] (VST_YUV_444),
 * [H][(W+1)/2] (VST_YUV_422) or [(H+1)/2][(W+1)/2] (4:2:0).  Any H, W >= 1 with H * W <= VST_MAX_FRAME_PIXELS; depth 9..16.
 *   layout  those of the raw video edge, and VST_YUV_422: chroma horizontally on the even luma columns, one sample per row.
 *           The value is additive: vst_yuv_to_rgb_u8 and vst_rgb_to_yuv_u8 go on refusing it.
 *   matrix  as above.
 *   range   with s = 2^(depth - 8): VST_YUV_LIMITED: Y offset yoff = 16 s, Y scale ys = 219 s, chroma scale cs = 224 s;
 *           VST_YUV_FULL: 0, 2^depth - 1, 2^depth - 1.  Chroma offset coff = 2^(depth - 1) in both.
 * vst_yuv16_to_rgb_f32: a code is first limited to 2^depth - 1; y' = (Y - yoff) / ys, pb = (U - coff) / cs, pr = (V - coff) / cs;
 *   R, G, B from the matrix expressions of vst_yuv_to_rgb_u8, clamped to [0, 1] and stored as fp32 with no quantisation.  If
 *   rgb_hwc_u8 is not NULL the same pixel is also written there as the byte floor(255 v + 0.5): the frame that label maps,
 *   mattes and the uint8 luminance route read.  4:2:0: U and V sampled bilinearly on the raw codes with the taps of the 8-bit
 *   kernel; 4:2:2: horizontally only - the chroma coordinate of luma x is x / 2 -, neighbours clamped to the plane.
 * vst_rgb_f32_to_yuv16: R, G, B clamped to [0, 1]; Y = Kr R + Kg G + Kb B, Cb = (B - Y) / (2 (1 - Kb)), Cr = (R - Y) / (2 (1 -
 *   Kr)); codes clamp(floor(yoff + Y ys + 0.5), 0, 2^depth - 1) and clamp(floor(coff + C cs + 0.5), 0, 2^depth - 1): round to
 *   nearest at the target depth (an extension: the reference only has the 8-bit truncation).  Chroma is reduced in float before
 *   that one rounding: 4:2:0 as in vst_rgb_to_yuv_u8; 4:2:2 with [1/4, 1/2, 1/4] around the even column and no vertical step; a
 *   missing neighbour is the edge pixel again.
 * fp64 arithmetic per pixel with one rounding at the end: a code or byte equals floor(v + 0.5) of the exact value v unless v
 * lies within 2^-20 of a tie, and an fp32 value is the exact one rounded once (tests/yuv16_ref.py).
 * VST_E_ARG for a null pointer (rgb_hwc_u8 excepted), depth outside 9..16, an unknown layout / matrix / range, H or W < 1 or
 * H * W past VST_MAX_FRAME_PIXELS; checks come before any launch.  Pointers need their type's alignment (2 bytes for the
 * planes) and nothing more: the planes of one flat Y|U|V buffer work for any H and W (aligned addresses take the wide paths). */
#define VST_YUV_422 3
int vst_yuv16_to_rgb_f32(const uint16_t* y, const uint16_t* u, const uint16_t* v, int H, int W, int depth, int layout,
                         int matrix, int range, float* rgb_planar /*[3][H][W]*/, uint8_t* rgb_hwc_u8 /*[H][W][3] or NULL*/,
                         void* stream);
int vst_rgb_f32_to_yuv16(const float* rgb_planar /*[3][H][W]*/, int H, int W, int depth, int layout, int matrix, int range,
                         uint16_t* y, uint16_t* u, uint16_t* v, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Deep resize (version 115; DESIGN.md section 6, "Deep resize"): utils.utils.img_resize restated in float, fused with
 * vst_yuv16_to_rgb_f32, so that a high-bit-depth frame of any size reaches the encoder at the stylised size.
 *
 * The arithmetic.  The frame is the clamped RGB of vst_yuv16_to_rgb_f32 at the source size Ws x Hs.  steps_wh = int[nsteps][2]
 * are the target sizes (w, h) of img_resize's resizes, in order (0 <= nsteps <= 4).  A step whose size differs from its input's
 * is a horizontal pass (if the width changes), then a vertical pass (if the height changes); an axis that does not change has
 * no pass and a step that changes nothing is skipped.  Every pass is out[i] = sum_j w[i][j] in[first_i + j] with Pillow's
 * NORMALISED DOUBLE weights - vst_resize_coeffs_f64: the bicubic kernel a = -0.5, support 2 * max(1, in/out), Pillow's window
 * and argument t * (1 / filterscale), the row divided by its sum; the numbers vst_resize_coeffs_u8 rounds to 22 bits, unrounded -
 * on fp32 elements with fp64 accumulation, the result rounded to fp32 once per pass.  Nothing is clamped or quantised between
 * passes or steps.  The last pass's value is clamped to [0, 1] and stored as fp32 in out_f32 = float [3][H][W]; if out_u8 is not
 * NULL, out_u8 = uint8 [H][W][3] also gets floor(255 v + 0.5) of that STORED fp32 value v, evaluated in double.  With no pass at
 * all the call is vst_yuv16_to_rgb_f32 into out_f32 / out_u8.
 *
 * vst_resize_coeffs_f64 : host only.  The table of one axis: bounds = int[out][2] = {first input index, number of taps}, w =
 *                        double[out][ksize] (taps past a row's count are 0), ksize = 2 * ceil(2 * max(1, in/out)) + 1.  *ksize
 *                        is always written; with bounds == NULL or w == NULL nothing else is (size query).  Checks and errors
 *                        as vst_resize_coeffs_u8.
 * tables_dev            : the passes' tables in the passes' order, on the device, on an 8-byte address: per pass its bounds (2 *
 *                        out words) followed by its weights (out * ksize doubles).
 * work                  : vst_yuv16_img_resize_workspace_bytes bytes on the device (the passes' intermediates; may be NULL when
 *                        that is 0: at most one pass, and that one horizontal).  One workspace serves one frame at a time.
 *                        workspace: 256-byte aligned, as every allocator here returns it.
 * Where the first pass is horizontal it reads the 16-bit planes itself (a workgroup converts the source span of its output tile
 * into LDS and filters from there: no source-size RGB frame exists); where it is vertical, vst_yuv16_to_rgb_f32 runs at the
 * source size into the workspace and plain passes follow.  The result is the one defined above either way.
 * Every launch is queued on `stream`; nothing synchronises.  Sizes only shrink: VST_E_SHAPE for a step larger than its input in
 * either axis or smaller by more than VST_RESIZE_MAX_SHRINK (16); VST_E_ARG for a
 * null pointer (out_u8 excepted), nsteps outside 0..4, a non-positive size, a misaligned table, and whatever vst_yuv16_to_rgb_f32
 * refuses.  All checks come before any launch.  Planes need 2-byte alignment and nothing more. */
int vst_resize_coeffs_f64(int in_size, int out_size, int* ksize, int* bounds, double* w);
int vst_yuv16_img_resize_workspace_bytes(int Hs, int Ws, int nsteps, const int* steps_wh, size_t* bytes);
int vst_yuv16_img_resize_f32(const uint16_t* y, const uint16_t* u, const uint16_t* v, int Hs, int Ws, int depth, int layout,
                             int matrix, int range, int nsteps, const int* steps_wh /*host, [nsteps][2] = (w, h)*/,
                             const void* tables_dev, float* work, float* out_f32 /*[3][H][W]*/,
                             uint8_t* out_u8 /*[H][W][3] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Guided upscale (version 116; csrc/guided.hip; DESIGN.md section 6, "Guided upscale"): He and Sun's fast guided filter with a
 * colour guide, which carries a stylisation made at a working size h x w over to a source frame of the full size H x W.  An
 * extension: the reference has no counterpart.
 *
 * The fit, at the working size.  I = guide / 255 (uint8 [h][w][3]), p = target (float [3][h][w]).  The box of a pixel is the
 * (2 radius + 1)^2 window around it clipped to the image, and a box mean divides by the number of pixels inside.  Per pixel:
 * mean_I, mean_p, Sigma = mean(I I^T) - mean_I mean_I^T, C = mean(I p^T) - mean_I mean_p^T, A = (Sigma + eps 1)^-1 C (3x3,
 * column c serves output channel c), b = mean_p - A^T mean_I.  coef = float [12][h][w] is the box mean, same clipped box, of
 * A[k][c] (plane 3 k + c) and b[c] (plane 9 + c).  Window sums and the solve are fp64; coef is the result rounded to fp32.
 *
 * The apply, at the full size.  The 12 planes are sampled bilinearly with half-pixel centres, x = (X + 0.5) w / W - 0.5 clamped
 * to [0, w - 1] and likewise in y (coordinates in double, weights and everything behind them fp32), and q[c] = b[c] + sum_k
 * A[k][c] src[k] / 255 with src = uint8 [H][W][3].  _f32 stores q as float [3][H][W]; _u8 stores uint8 [H][W][3] under the
 * writer's epilogue of vst_resize_f32_to_u8: * 255, clamp to [0, 255], truncate, NaN -> 0.
 *
 * vst_guided_workspace_bytes : host only; the bytes vst_guided_fit needs at `ws` (device memory on an 8-byte address; one workspace
 *                              serves one fit at a time).
 * radius is 1..VST_GUIDED_MAX_RADIUS and 48 h w < 2^31, VST_E_SHAPE otherwise; the apply needs H >= h and W >= w (equal sizes are
 * the plain guided filter) and an output of fewer than 2^31 bytes, VST_E_SHAPE otherwise.  VST_E_ARG for a null pointer, a
 * non-positive size, an eps that is not positive and finite, a pointer off its type's alignment; VST_E_WORKSPACE for a null
 * workspace.  Nothing is allocated; every launch is queued on `stream`; all checks come before any launch. */
#define VST_GUIDED_MAX_RADIUS 8
int vst_guided_workspace_bytes(int h, int w, int radius, size_t* bytes);
int vst_guided_fit(const uint8_t* guide_u8_hwc, const float* target_f32_planar, int h, int w, int radius, double eps,
                   float* coef_f32 /*[12][h][w]*/, void* ws, void* stream);
int vst_guided_apply_u8(const float* coef, int h, int w, const uint8_t* src_u8_hwc, int H, int W, uint8_t* dst_u8_hwc,
                        void* stream);
int vst_guided_apply_f32(const float* coef, int h, int w, const uint8_t* src_u8_hwc, int H, int W, float* dst_f32_planar,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Affinity loss (version 117; csrc/matting.hip; DESIGN.md section 6, "Affinity loss"): the reference's Matting-Laplacian loss of
 * a stylised image x against its content image, and its gradient, without the matrix.  Replaces compute_laplacian
 * (utils/MattingLaplacian.py:15-81: the sparse HW x HW matrix L built on the host) and laplacian_loss_grad
 * (utils/MattingLaplacian.py:84-96, called at train.py:163-173: torch.mm of L with every channel).
 *
 * I = guide / 255 (uint8 [h][w][3]).  x is float [3][h][w] (_f32: the stylised frame before the writer's epilogue) or uint8
 * [h][w][3] read as v / 255 (_u8: a written frame).  A window k is the n = (2 radius + 1)^2 pixels around a centre at least
 * `radius` from every edge (windows fully inside the image, as in the reference).  With mu_k the window mean of I, S_k its
 * population covariance, inv_k = (S_k + (eps / n) 1)^-1 and, per channel c, m_k the window mean of x_c and v_k = cov_k(I, x_c):
 *
 *     (L x_c)_i   = sum over the windows k that hold i of   x_i - m_k - (I_i - mu_k)^T inv_k v_k
 *     x_c^T L x_c = sum_i x_i (L x_c)_i                   ( = sum_k n (var_k(x_c) - v_k^T inv_k v_k) )
 *     loss3[c]    = x_c^T L x_c / (h w)                     grad[c] = 2 L x_c / (h w)   (float [3][h][w]; NULL: not written)
 *
 * The sum of loss3 is the reference's loss, grad its second return value.  Every moment, the 3x3 inverse, the residuals and the
 * sums are fp64 (inv_k v_k by an L D L^T solve: a window across an edge between flat regions has a rank-one S_k, which costs a
 * cofactor inverse the square of the condition); moments are taken relative to the window's centre pixel, so a flat window has
 * S_k = 0 exactly and a constant x gives exactly 0.  Each workgroup leaves three partial sums in `ws` and a second launch adds them in a fixed order: no
 * floating-point atomics, and two runs on the same input give the same bits.
 *
 * vst_matting_workspace_bytes : host only; the bytes the two calls need at `ws` (device memory on an 8-byte address; one
 *                               workspace serves one call at a time).
 * VST_E_SHAPE unless 1 <= radius <= VST_MATTING_MAX_RADIUS, h, w >= 2 radius + 1 and h w <= VST_MAX_FRAME_PIXELS.  VST_E_ARG for
 * a null pointer other than grad, an eps that is not positive and finite, a pointer off its type's alignment (loss3 and ws: 8
 * bytes).  Nothing is allocated; both launches are queued on `stream` (a hipStream_t, as everywhere here); nothing
 * synchronises; all checks come before any launch. */
#define VST_MATTING_MAX_RADIUS 3
int vst_matting_workspace_bytes(int h, int w, int radius, size_t* bytes);
int vst_matting_loss_f32(const uint8_t* guide_u8_hwc, const float* x_f32_planar, int h, int w, int radius, double eps,
                         double* loss3, float* grad_f32_planar_or_null, void* ws, void* stream);
int vst_matting_loss_u8(const uint8_t* guide_u8_hwc, const uint8_t* x_u8_hwc, int h, int w, int radius, double eps,
                        double* loss3, float* grad_f32_planar_or_null, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal loss (version 118; csrc/temporal.hip; DESIGN.md section 6, "Temporal loss"): the reference's utils/TemporalLoss.py on the
 * device - warp(x, flo), mean |warp(first, flow) - second|, and the smooth random flow of GenerateFakeFlow.
 *
 * Frames are uint8 [h][w][3] (_u8) or float [3][h][w] (_f32); a flow is float [2][h][w], x displacement first; NULL: no warp.
 *
 * vst_warp_* : dst(y, x) = src(sy, sx) [+ noise], the reference's grid_sample(mode='nearest', padding_mode='border') with its
 *   quirk kept: the grid is normalised by n - 1 but sampled with align_corners=False.  Per axis of n pixels, in fp32, each
 *   operation rounded on its own (no fused multiply-add), in this order:
 *       v = p - flo;  t = 2 v / max(n - 1, 1) - 1;  i = ((t + 1) n - 1) / 2;  i = min(max(i, 0), n - 1);  s = nearbyint(i)
 *   (ties to even).  noise (float [3][h][w], NULL: none) is added after the warp: _f32: v + noise; _u8:
 *   min(max(rint((float)v + 255.0f noise), 0), 255) in fp32, again without contraction.  src and dst must differ.
 * vst_temporal_l1_* : loss3[c] = mean over the pixels of |warp(a, flow)_c - b_c| (the reference's scalar is the mean of the
 *   three), with the warp fused in; `warped` (NULL: not written; never a or b) receives warp(a, flow), the reference's second
 *   return value.  _u8: the sum is an exact integer, divided once by 255.0 h w in fp64.  _f32: differences and sums in fp64.
 *   Each workgroup leaves three partial sums in `ws`, a second launch adds them in a fixed order: no floating-point atomics,
 *   and two runs on the same input give the same bits.
 * vst_temporal_workspace_bytes : host only; the bytes the two calls need at `ws` (device memory on an 8-byte address; one
 *   workspace serves one call at a time).
 * vst_fake_flow : the motion_level > 0 branch of GenerateFakeFlow from a coarse grid drawn by the caller: grid (DEVICE memory,
 *   double [gh][gw][2]) is upsampled to [h][w] by the INTER_LINEAR rule (source coordinate (d + 0.5) src / dst - 0.5, edges
 *   replicated), shift_x / shift_y are added, and a ksize x ksize box filter with anchor ksize / 2 (window x - ksize / 2 ..
 *   x - ksize / 2 + ksize - 1) and BORDER_REFLECT_101 follows; fp64 throughout, rounded once to float [2][h][w].  The reference's
 *   values are gh = h / 100, gw = w / 100, ksize = 100.  vst_fake_flow_workspace_bytes: host only, the bytes at `ws`.
 *
 * VST_E_SHAPE unless h, w >= 1 and h w <= VST_MAX_FRAME_PIXELS, and for the flow 1 <= gh, gw <= VST_FAKE_FLOW_MAX_GRID and
 * 1 <= ksize <= min(h, w).  VST_E_ARG for a null pointer other than those named optional, a pointer off its type's alignment
 * (loss3, ws, grid: 8 bytes), aliased frames, a shift that is not finite.  Nothing is allocated; every launch is queued on `stream`;
 * nothing synchronises; all checks come before any launch. */
#define VST_FAKE_FLOW_MAX_GRID 1024
int vst_warp_u8(const uint8_t* src_u8_hwc, const float* flow_or_null, const float* noise_or_null, uint8_t* dst_u8_hwc, int h, int w,
                void* stream);
int vst_warp_f32(const float* src_f32_planar, const float* flow_or_null, const float* noise_or_null, float* dst_f32_planar, int h,
                 int w, void* stream);
int vst_temporal_workspace_bytes(int h, int w, size_t* bytes);
int vst_temporal_l1_u8(const uint8_t* a_u8_hwc, const uint8_t* b_u8_hwc, const float* flow_or_null, int h, int w, double* loss3,
                       uint8_t* warped_or_null, void* ws, void* stream);
int vst_temporal_l1_f32(const float* a_f32_planar, const float* b_f32_planar, const float* flow_or_null, int h, int w, double* loss3,
                        float* warped_or_null, void* ws, void* stream);
int vst_fake_flow_workspace_bytes(int h, int w, int gh, int gw, int ksize, size_t* bytes);
int vst_fake_flow(const double* grid_f64, int gh, int gw, double shift_x, double shift_y, int ksize, float* flow_f32, int h, int w,
                  void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optical flow (version 119; csrc/flow.hip; DESIGN.md section 6, "Optical flow"): a dense coarse-to-fine, warping Lucas-Kanade
 * estimator on a pair of uint8 frames, the forward-backward consistency mask, and the temporal L1 over the mask's pixels.
 *
 * vst_flow_lk_u8 : ref (frame t) and src (frame t-1), uint8 [h][w][3] -> flow, float [2][h][w], x displacement first, in the
 *   convention of vst_warp_* and vst_temporal_l1_*: ref(p) ~ src(p - flow(p)).  The kernels estimate d = -flow, ref(q) ~
 *   src(q + d(q)), all in fp64 without fused multiply-adds, and round once to fp32:
 *     grey      g = (0.299 r + 0.587 g + 0.114 b) / 255.
 *     pyramid   level 0 is the frame; level l+1 has ceil(h_l / 2) x ceil(w_l / 2) pixels and is pixel (2y, 2x) of level l after
 *               the separable 5-tap binomial filter [1 4 6 4 1] / 16 (rows, then columns; edges replicated).  A level is added
 *               while fewer than `levels` exist and the new level's shorter edge is at least 8.
 *     field     d = 0 at the coarsest level; going down, d_l(y, x) = 2 bilinear(d_{l+1}; y / 2, x / 2).  bilinear(A; y, x) clamps
 *               each coordinate to [0, n - 1], takes x0 = floor(x), x1 = min(x0 + 1, n - 1), fx = x - x0 (y alike) and returns
 *               (1 - fy) ((1 - fx) A[y0][x0] + fx A[y0][x1]) + fy ((1 - fx) A[y1][x0] + fx A[y1][x1]).
 *     tensor    per level, Rx = (R(y, x+1) - R(y, x-1)) / 2, Ry alike, edges replicated; over the (2 radius + 1)^2 window with
 *               its coordinates clamped to the frame, A11 = sum Rx^2 + lambda, A12 = sum Rx Ry, A22 = sum Ry^2 + lambda (lambda
 *               enters once, here: A is the regularised matrix the update inverts).
 *     iterate   `iters` times per level: e(q) = (bilinear(S; y + dy(q), x + dx(q)) - R(q)) my mx, where m = min(max(1 - o, 0), 1)
 *               per axis and o = max(-c, c - (n - 1), 0) is how far the unclamped sample coordinate c lies outside the frame;
 *               b1 = sum Rx e, b2 = sum Ry e over the same window; delta = -A^-1 b by the closed form (det = A11 A22 - A12^2,
 *               delta_x = -(A22 b1 - A12 b2) / det, delta_y = -(A11 b2 - A12 b1) / det), each component clamped to [-1, 1];
 *               d += delta; d = binomial5(d) per component (the pyramid's filter).
 *     finish    flow = -d_0, rounded to float.
 *   No floating-point atomics: two runs on the same input give the same bits.
 * vst_flow_workspace_bytes : host only; the bytes vst_flow_lk_u8 needs at `ws` (device memory on an 8-byte address; one
 *   workspace serves one call at a time): 4 fp64 planes per pyramid level and 7 at the frame's size.
 * vst_flow_consistency : flow_fwd = the flow of (ref = t, src = t-1), flow_bwd = the flow of the swapped pair.  With q = p -
 *   fwd(p) and b = bilinear(bwd; q) in fp64, valid(p) = 1 iff q lies inside [0, h-1] x [0, w-1] and |fwd(p) + b|^2 <=
 *   0.01 (|fwd(p)|^2 + |b|^2) + 0.5 (Sundaram, Brox and Keutzer, ECCV 2010); else 0.  valid: uint8 [h][w].
 * vst_temporal_l1_masked_u8 : vst_temporal_l1_u8 over the pixels with valid != 0: loss4[c] = the exact integer sum of channel c
 *   divided once by 255.0 count in fp64, loss4[3] = count / (h w); count = 0: four zeros.  `warped` (NULL: not written) receives
 *   warp(a, flow) at every pixel, valid or not.  The same two launches and fixed-order sums; `ws` is that of
 *   vst_temporal_workspace_bytes.
 *
 * VST_E_SHAPE unless h, w >= 8 and h w <= VST_MAX_FRAME_PIXELS, 1 <= levels <= VST_FLOW_MAX_LEVELS, 1 <= iters <=
 * VST_FLOW_MAX_ITERS, 1 <= radius <= VST_FLOW_MAX_RADIUS.  VST_E_ARG for a null pointer other than those named optional, a pointer
 * off its type's alignment (ws, loss4: 8 bytes), an output that overlaps an input or the workspace, a lambda that is not finite
 * and > 0.  Nothing is allocated; every launch is queued on `stream`; nothing synchronises; all checks come before any launch. */
#define VST_FLOW_MAX_LEVELS 8
#define VST_FLOW_MAX_ITERS 16
#define VST_FLOW_MAX_RADIUS 7
int vst_flow_workspace_bytes(int h, int w, int levels, size_t* bytes);
int vst_flow_lk_u8(const uint8_t* ref_u8_hwc, const uint8_t* src_u8_hwc, int h, int w, int levels, int iters, int radius,
                   double lambda, float* flow_f32, void* ws, void* stream);
int vst_flow_consistency(const float* flow_fwd, const float* flow_bwd, int h, int w, uint8_t* valid, void* stream);
int vst_temporal_l1_masked_u8(const uint8_t* a_u8_hwc, const uint8_t* b_u8_hwc, const float* flow_or_null, const uint8_t* valid,
                              int h, int w, double* loss4, uint8_t* warped_or_null, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stabiliser (version 121; csrc/stabilise.hip; DESIGN.md section 6, "Stabiliser"): a flow-guided recursive blend of the frame that
 * is about to be written with the frame written before it.  All frames are uint8 [h][w][3]; flow is float [2][h][w], x first, in
 * the convention of vst_flow_lk_u8: frame t at p ~ frame t-1 at p - flow(p); valid (NULL: every pixel) is uint8 [h][w], the mask
 * of vst_flow_consistency.  One thread per pixel, fp64 without fused multiply-adds, with S = cur_out:
 *     sample    q = p - flow(p) in fp64; inside = q in [0, w-1] x [0, h-1] (false for NaN and +-inf); live = inside and
 *               (valid == NULL or valid(p) != 0).  Not live: written(p) = S(p), and nothing is read at q.
 *     warp      I~ = bilinear(prev_in; q), O~ = bilinear(prev_written; q) per channel on the 0..255 scale, with the bilinear of
 *               the "Optical flow" section: (1 - ay) ((1 - ax) a00 + ax a01) + ay ((1 - ax) a10 + ax a11).
 *     weight    d_c = cur_in_c(p) - I~_c; e = ((d_0^2 + d_1^2) + d_2^2) / 3; wgt = gain / (1 + e / sigma^2): where the input
 *               changed along the flow (an occlusion, a wrong flow, a change of light) the weight falls off.
 *     blend     delta = min(max(wgt (O~_c - S_c), -limit), limit); written_c = min(max(rint(S_c + delta), 0), 255), rint to even.
 *   Only + - * /, comparisons and rint: every step is correctly rounded, and a numpy statement of the same steps gives the same
 *   bytes.  No workspace, no atomics.
 *
 * VST_E_SHAPE unless h, w >= 1 and h w <= VST_MAX_FRAME_PIXELS.  VST_E_ARG for a null pointer other than valid, a flow off the
 * float grid, gain outside (0, 1), sigma not in (0, inf), limit not in [0, inf), `written` overlapping any input (prev_written and
 * cur_out included: the blend is never in place).  Queued on `stream`; nothing synchronises; all checks come before the launch. */
int vst_stabilise_u8(const uint8_t* cur_in, const uint8_t* prev_in, const uint8_t* cur_out, const uint8_t* prev_written,
                     const float* flow, const uint8_t* valid_or_null, int h, int w, double gain, double sigma, double limit,
                     uint8_t* written, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* VSTNET_H */
