// Whole passes of the reversible network on the coupling blocks of conv.hip / conv3.hip: forward (image -> z), inverse
// (z -> image), and the packed-code forms encode / decode / masked decode (RevResNet._forward / _inverse,
// models/RevResNet.py:210-239).
#include "common.h"

static const int kBlockChannel[VST_NUM_BLOCKS] = {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 64, 64, 64, 64, 64, 64,
                                                  64, 64, 64, 64, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256,
                                                  256, 256};
static const int kBlockStride[VST_NUM_BLOCKS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1,
                                                 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

// Images per internal sub-batch: the reversible state + intermediates of a sub-batch (160 B/pixel) should stay in
// the 256 MiB Infinity Cache between the 96 conv launches of a pass (measured: 8 frames of 1024x1024 in one batch
// run 27 % slower per frame than one at a time); small images are still batched to fill the chip.
static int pass_sub_batch(int B, int H, int W) {
    const size_t per_img = (size_t)H * W * 288;
    size_t nb = ((size_t)192 << 20) / per_img;
    if (nb < 1) nb = 1;
    return nb > (size_t)B ? B : (int)nb;
}

// the 32 coupling blocks of a forward pass on the state halves s[0], s[1] (n images each), input packing included
static int forward_blocks(const vst_net_weights* w, const float* x, const uint8_t* x_u8, float* const s[2], float* tmp, int B,
                          int C_in, int H, int W, int precision, void* stream) {
    // forward block 0 has x2 = 0: F(0) is a per-channel constant that the pack kernel adds (fp32 diagnostic mode keeps
    // the literal three convolutions)
    const bool fold0 = precision != VST_PREC_FP32;
    float* k16 = tmp;                                        // 16 floats at the head of the intermediates' scratch
    int rc = fold0 ? vst_block0_const(&w->blocks[0], k16, stream) : VST_OK;
    if (rc) return rc;
    rc = vst_pack_input_k(x, x_u8, s[0], s[1], B, x_u8 ? 3 : C_in, H, W, fold0 ? k16 : nullptr, stream);
    if (rc) return rc;
    const bool sp = vst_is_f16(precision);
    for (int k = fold0 ? 1 : 0; k < VST_NUM_BLOCKS; ++k) {
        if (sp && k >= 21)      // block k's conv.7 leaves the split planes of its dst = block k+1's src
            rc = vst3_block256(&w->blocks[k], +1, precision, s[k & 1], s[1 - (k & 1)], tmp, k - 21, 1, B, H, W, stream);
        else
            rc = vst_block_apply(&w->blocks[k], kBlockChannel[k], kBlockStride[k], +1, precision, s[k & 1], s[1 - (k & 1)],
                                 tmp, B, H, W, stream);
        if (rc) return rc;
    }
    return VST_OK;
}

// the 32 coupling blocks of an inverse pass on the state halves (f16x2: s[0] is given as split planes in plane buffer 0 of
// tmp - block 31 reads its src only through them and block 30 takes its old values from them too), output unpacking included
static int inverse_blocks(const vst_net_weights* w, float* x, uint8_t* x_u8, float* const s[2], float* tmp, int B, int C_out,
                          int H, int W, int precision, void* stream) {
    const bool sp = vst_is_f16(precision);
    int rc = VST_OK;
    // block 0 in an MFMA mode: its pair launch writes the image (no state write, no unpack launch)
    const bool rgb0 = precision != VST_PREC_FP32 && vst_option(VST_OPT_OUT_RGB);
    if (rgb0) {
        if ((!x && !x_u8) || !vst_shape_ok(B, H, W) || (!x_u8 && (C_out < 1 || C_out > 16))) return VST_E_ARG;
        for (int i = 0; i < 3; ++i)
            if (!w->blocks[0].conv[i].packed || !w->blocks[0].conv[i].bias) return VST_E_ARG;
    }
    for (int k = VST_NUM_BLOCKS - 1; k >= 0; --k) {
        if (sp && k >= 21)
            rc = vst3_block256(&w->blocks[k], -1, precision, s[k & 1], s[1 - (k & 1)], tmp, VST_NUM_BLOCKS - 1 - k, 1, B, H, W,
                               stream);
        else if (k == 0 && rgb0)
            return vst_block0_to_image(&w->blocks[0], precision, s[0], s[1], tmp, B, H, W, x_u8 ? nullptr : x, x_u8, C_out, stream);
        else
            rc = vst_block_apply(&w->blocks[k], kBlockChannel[k], kBlockStride[k], -1, precision, s[k & 1], s[1 - (k & 1)],
                                 tmp, B, H, W, stream);
        if (rc) return rc;
    }
    return x_u8 ? vst_unpack_output_u8(s[0], x_u8, B, H, W, stream) : vst_unpack_output(s[0], x, B, C_out, H, W, stream);
}

// A pass runs in sub-batches of pass_sub_batch images on one workspace: [state half 0 | state half 1 | block scratch].
static int revnet_forward_any(const vst_net_weights* w, const float* x, const uint8_t* x_u8, float* z, void* workspace,
                              int B, int C_in, int H, int W, int sp_steps, int precision, void* stream) {
    if (!w || (!x && !x_u8) || !z) return VST_E_ARG;
    if (!workspace) return VST_E_WORKSPACE;
    if (!vst_shape_ok(B, H, W) || C_in < 1 || C_in > 16) return VST_E_SHAPE;
    if (sp_steps != 1 && sp_steps != 2) return VST_E_MODE;
    const int nb = pass_sub_batch(B, H, W);
    const size_t zimg = (size_t)32 * H * W;                 // floats per image of z in both modes
    for (int b0 = 0; b0 < B; b0 += nb) {
        const int n = B - b0 < nb ? B - b0 : nb;
        float* s[2] = {(float*)workspace, (float*)workspace + n * (zimg / 2)};
        float* tmp = s[1] + n * (zimg / 2);
        int rc = forward_blocks(w, x ? x + (size_t)b0 * C_in * H * W : nullptr, x_u8 ? x_u8 + (size_t)b0 * H * W * 3 : nullptr, s,
                                tmp, n, C_in, H, W, precision, stream);
        if (!rc) rc = vst_spread(s[0], s[1], z + b0 * zimg, n, H, W, sp_steps, stream);
        if (rc) return rc;
    }
    return VST_OK;
}

static int revnet_inverse_any(const vst_net_weights* w, const float* z, float* x, uint8_t* x_u8, void* workspace, int B,
                              int C_out, int H, int W, int sp_steps, int precision, void* stream) {
    if (!w || (!x && !x_u8) || !z) return VST_E_ARG;
    if (!workspace) return VST_E_WORKSPACE;
    if (!vst_shape_ok(B, H, W) || C_out < 1 || C_out > 16) return VST_E_SHAPE;
    if (sp_steps != 1 && sp_steps != 2) return VST_E_MODE;
    const int nb = pass_sub_batch(B, H, W);
    const size_t zimg = (size_t)32 * H * W;
    for (int b0 = 0; b0 < B; b0 += nb) {
        const int n = B - b0 < nb ? B - b0 : nb;
        float* s[2] = {(float*)workspace, (float*)workspace + n * (zimg / 2)};
        float* tmp = s[1] + n * (zimg / 2);
        // f16x2: the gather writes s[0] straight into plane buffer 0 (no fp32 copy, no pre-split pass)
        int rc = vst_is_f16(precision)
                     ? vst3_gather_planes(z + b0 * zimg, vst3_plane_buffer(tmp, 0, n, H, W), s[1], n, H, W, sp_steps, stream)
                     : vst_gather(z + b0 * zimg, s[0], s[1], n, H, W, sp_steps, stream);
        if (!rc) rc = inverse_blocks(w, x ? x + (size_t)b0 * C_out * H * W : nullptr, x_u8 ? x_u8 + (size_t)b0 * H * W * 3 : nullptr,
                                     s, tmp, n, C_out, H, W, precision, stream);
        if (rc) return rc;
    }
    return VST_OK;
}

// Packed code (photorealistic mode): the state halves themselves, per image [2][H/4][W/4][256] floats = one 32-float row per
// full-resolution pixel.  encode = forward pass without the spread, one image at a time (its halves are the pass's state
// buffers); decode = [affine map of an unmasked cWCT on the rows ->] inverse pass without the gather.
static int revnet_encode_any(const vst_net_weights* w, const float* x, const uint8_t* x_u8, float* code, void* workspace, int B,
                             int C_in, int H, int W, int precision, void* stream) {
    if (!w || (!x && !x_u8) || !code) return VST_E_ARG;
    if (!workspace) return VST_E_WORKSPACE;
    if (!vst_shape_ok(B, H, W) || C_in < 1 || C_in > 16) return VST_E_SHAPE;
    const size_t img = (size_t)32 * H * W;
    float* tmp = (float*)workspace + img;                    // the scratch part of a one-image pass workspace
    for (int b = 0; b < B; ++b) {
        float* s[2] = {code + b * img, code + b * img + img / 2};
        const int rc = forward_blocks(w, x ? x + (size_t)b * C_in * H * W : nullptr, x_u8 ? x_u8 + (size_t)b * H * W * 3 : nullptr,
                                      s, tmp, 1, C_in, H, W, precision, stream);
        if (rc) return rc;
    }
    return VST_OK;
}

// one image whose cWCT is a masked one: a map per row (label slot), cwct.hip: vst3_apply_labels_code
static int revnet_decode_labels_any(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                                    const void* plan, int max_slots, const float* strength_rows, float* x, uint8_t* x_u8,
                                    void* workspace, int C_out, int H, int W, int precision, void* stream) {
    if (!w || (!x && !x_u8) || !code || !affines || !mask_rows || !plan) return VST_E_ARG;
    if (!workspace) return VST_E_WORKSPACE;
    if (!vst_shape_ok(1, H, W) || C_out < 1 || C_out > 16 || max_slots < 1 || max_slots > 8) return VST_E_SHAPE;
    const size_t img = (size_t)32 * H * W;
    float* s[2] = {(float*)workspace, (float*)workspace + img / 2};
    float* tmp = (float*)workspace + img;
    unsigned char* planes0 = vst_is_f16(precision) ? vst3_plane_buffer(tmp, 0, 1, H, W) : nullptr;
    int rc = vst3_apply_labels_code(code, s[0], s[1], planes0, H, W, affines, mask_rows, plan, max_slots, strength_rows, stream);
    if (rc) return rc;
    return inverse_blocks(w, x, x_u8, s, tmp, 1, C_out, H, W, precision, stream);
}

// strength_rows (nullable): float[B][rows of one image], blended in by the apply; without affines A(x) = x and nothing blends.
// K > 0 (style maps): affines = float[B][K][N*N+N] and weight_rows = float[B][K][rows], applied by vst3_apply_code_mix
static int revnet_decode_any(const vst_net_weights* w, const float* code, const float* affines, const float* strength_rows,
                             float* x, uint8_t* x_u8, void* workspace, int B, int C_out, int H, int W, int sp_steps, int precision,
                             void* stream, int K = 0, const float* weight_rows = nullptr) {
    if (!w || (!x && !x_u8) || !code) return VST_E_ARG;
    if (K != 0 && (K < 2 || K > CWCT_MAX_STYLES || !affines || !weight_rows)) return VST_E_ARG;
    if (!workspace) return VST_E_WORKSPACE;
    if (!vst_shape_ok(B, H, W) || C_out < 1 || C_out > 16) return VST_E_SHAPE;
    if (sp_steps != 1 && sp_steps != 2) return VST_E_MODE;
    if (K != 0 && sp_steps == 1 && K != 2) return VST_E_MODE;
    const int N = sp_steps == 2 ? 32 : 128;
    const size_t img = (size_t)32 * H * W, rows = img / N;
    float* s[2] = {(float*)workspace, (float*)workspace + img / 2};
    float* tmp = (float*)workspace + img;
    const bool sp = vst_is_f16(precision);
    unsigned char* planes0 = sp ? vst3_plane_buffer(tmp, 0, 1, H, W) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < B; ++b) {
        const float* c = code + b * img;
        int rc;
        if (K) {
            rc = vst3_apply_code_mix(c, s[0], s[1], planes0, H, W, sp_steps, affines + (size_t)b * K * ((size_t)N * N + N), K,
                                     weight_rows + (size_t)b * K * rows, strength_rows ? strength_rows + (size_t)b * rows : nullptr,
                                     stream);
        } else if (affines) {
            rc = vst3_apply_code(c, s[0], s[1], planes0, H, W, sp_steps, affines + (size_t)b * ((size_t)N * N + N),
                                 strength_rows ? strength_rows + (size_t)b * rows : nullptr, stream);
        } else {                                             // plain copy into the pass's state (it is updated in place)
            rc = sp ? vst3_presplit(c, planes0, 1, H, W, stream)
                    : (int)hipMemcpyAsync(s[0], c, img / 2 * sizeof(float), hipMemcpyDeviceToDevice, st);
            if (!rc) rc = (int)hipMemcpyAsync(s[1], c + img / 2, img / 2 * sizeof(float), hipMemcpyDeviceToDevice, st);
        }
        if (rc) return rc;
        rc = inverse_blocks(w, x ? x + (size_t)b * C_out * H * W : nullptr, x_u8 ? x_u8 + (size_t)b * H * W * 3 : nullptr, s, tmp,
                            1, C_out, H, W, precision, stream);
        if (rc) return rc;
    }
    return VST_OK;
}

extern "C" {

size_t vst_pass_workspace_bytes(int B, int H, int W) { return (size_t)B * H * W * (16 + 16 + 40) * sizeof(float); }

int vst_pass_sub_batch(int B, int H, int W) {
    if (!vst_shape_ok(B, H, W)) return VST_E_SHAPE;
    return pass_sub_batch(B, H, W);
}

int vst_revnet_forward(const vst_net_weights* w, const float* x, float* z, void* workspace, int B, int C_in, int H,
                       int W, int sp_steps, int precision, void* stream) {
    if (!x) return VST_E_ARG;
    return revnet_forward_any(w, x, nullptr, z, workspace, B, C_in, H, W, sp_steps, precision, stream);
}

int vst_revnet_inverse(const vst_net_weights* w, const float* z, float* x, void* workspace, int B, int C_out, int H,
                       int W, int sp_steps, int precision, void* stream) {
    if (!x) return VST_E_ARG;
    return revnet_inverse_any(w, z, x, nullptr, workspace, B, C_out, H, W, sp_steps, precision, stream);
}

int vst_revnet_forward_u8(const vst_net_weights* w, const uint8_t* frames_hwc, float* z, void* workspace, int B, int H,
                          int W, int sp_steps, int precision, void* stream) {
    if (!frames_hwc) return VST_E_ARG;
    return revnet_forward_any(w, nullptr, frames_hwc, z, workspace, B, 3, H, W, sp_steps, precision, stream);
}

int vst_revnet_inverse_u8(const vst_net_weights* w, const float* z, uint8_t* frames_hwc, void* workspace, int B, int H,
                          int W, int sp_steps, int precision, void* stream) {
    if (!frames_hwc) return VST_E_ARG;
    return revnet_inverse_any(w, z, nullptr, frames_hwc, workspace, B, 3, H, W, sp_steps, precision, stream);
}

int vst_revnet_encode(const vst_net_weights* w, const float* x, float* code, void* workspace, int B, int C_in, int H, int W,
                      int precision, void* stream) {
    if (!x) return VST_E_ARG;
    return revnet_encode_any(w, x, nullptr, code, workspace, B, C_in, H, W, precision, stream);
}

int vst_revnet_encode_u8(const vst_net_weights* w, const uint8_t* frames_hwc, float* code, void* workspace, int B, int H, int W,
                         int precision, void* stream) {
    if (!frames_hwc) return VST_E_ARG;
    return revnet_encode_any(w, nullptr, frames_hwc, code, workspace, B, 3, H, W, precision, stream);
}

int vst_revnet_decode_blend(const vst_net_weights* w, const float* code, const float* affines, const float* strength_rows,
                            float* x, void* workspace, int B, int C_out, int H, int W, int sp_steps, int precision, void* stream) {
    if (!x) return VST_E_ARG;
    return revnet_decode_any(w, code, affines, strength_rows, x, nullptr, workspace, B, C_out, H, W, sp_steps, precision, stream);
}

int vst_revnet_decode_blend_u8(const vst_net_weights* w, const float* code, const float* affines, const float* strength_rows,
                               uint8_t* frames_hwc, void* workspace, int B, int H, int W, int sp_steps, int precision,
                               void* stream) {
    if (!frames_hwc) return VST_E_ARG;
    return revnet_decode_any(w, code, affines, strength_rows, nullptr, frames_hwc, workspace, B, 3, H, W, sp_steps, precision,
                             stream);
}

int vst_revnet_decode_mix(const vst_net_weights* w, const float* code, const float* affines, int K, const float* weight_rows,
                          const float* strength_rows, float* x, void* workspace, int B, int C_out, int H, int W, int sp_steps,
                          int precision, void* stream) {
    if (!x || !affines || !weight_rows || K < 2 || K > CWCT_MAX_STYLES) return VST_E_ARG;
    return revnet_decode_any(w, code, affines, strength_rows, x, nullptr, workspace, B, C_out, H, W, sp_steps, precision, stream, K,
                             weight_rows);
}

int vst_revnet_decode_mix_u8(const vst_net_weights* w, const float* code, const float* affines, int K, const float* weight_rows,
                             const float* strength_rows, uint8_t* frames_hwc, void* workspace, int B, int H, int W, int sp_steps,
                             int precision, void* stream) {
    if (!frames_hwc || !affines || !weight_rows || K < 2 || K > CWCT_MAX_STYLES) return VST_E_ARG;
    return revnet_decode_any(w, code, affines, strength_rows, nullptr, frames_hwc, workspace, B, 3, H, W, sp_steps, precision,
                             stream, K, weight_rows);
}

int vst_revnet_decode(const vst_net_weights* w, const float* code, const float* affines, float* x, void* workspace, int B,
                      int C_out, int H, int W, int sp_steps, int precision, void* stream) {
    return vst_revnet_decode_blend(w, code, affines, nullptr, x, workspace, B, C_out, H, W, sp_steps, precision, stream);
}

int vst_revnet_decode_u8(const vst_net_weights* w, const float* code, const float* affines, uint8_t* frames_hwc, void* workspace,
                         int B, int H, int W, int sp_steps, int precision, void* stream) {
    return vst_revnet_decode_blend_u8(w, code, affines, nullptr, frames_hwc, workspace, B, H, W, sp_steps, precision, stream);
}

int vst_revnet_decode_labels_blend(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                                   const void* plan, int max_slots, const float* strength_rows, float* x, void* workspace,
                                   int C_out, int H, int W, int precision, void* stream) {
    if (!x) return VST_E_ARG;
    return revnet_decode_labels_any(w, code, affines, mask_rows, plan, max_slots, strength_rows, x, nullptr, workspace, C_out, H,
                                    W, precision, stream);
}

int vst_revnet_decode_labels_blend_u8(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                                      const void* plan, int max_slots, const float* strength_rows, uint8_t* frame_hwc,
                                      void* workspace, int H, int W, int precision, void* stream) {
    if (!frame_hwc) return VST_E_ARG;
    return revnet_decode_labels_any(w, code, affines, mask_rows, plan, max_slots, strength_rows, nullptr, frame_hwc, workspace, 3,
                                    H, W, precision, stream);
}

int vst_revnet_decode_labels(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                             const void* plan, int max_slots, float* x, void* workspace, int C_out, int H, int W, int precision,
                             void* stream) {
    return vst_revnet_decode_labels_blend(w, code, affines, mask_rows, plan, max_slots, nullptr, x, workspace, C_out, H, W,
                                          precision, stream);
}

int vst_revnet_decode_labels_u8(const vst_net_weights* w, const float* code, const float* affines, const uint8_t* mask_rows,
                                const void* plan, int max_slots, uint8_t* frame_hwc, void* workspace, int H, int W, int precision,
                                void* stream) {
    return vst_revnet_decode_labels_blend_u8(w, code, affines, mask_rows, plan, max_slots, nullptr, frame_hwc, workspace, H, W,
                                             precision, stream);
}

int vst_code_to_z(const float* code, float* z, int B, int H, int W, int sp_steps, void* stream) {
    if (!code || !z) return VST_E_ARG;
    const size_t img = (size_t)32 * H * W;
    for (int b = 0; b < B; ++b) {
        const int rc = vst_spread(code + b * img, code + b * img + img / 2, z + b * img, 1, H, W, sp_steps, stream);
        if (rc) return rc;
    }
    return VST_OK;
}

int vst_z_to_code(const float* z, float* code, int B, int H, int W, int sp_steps, void* stream) {
    if (!code || !z) return VST_E_ARG;
    const size_t img = (size_t)32 * H * W;
    for (int b = 0; b < B; ++b) {
        const int rc = vst_gather(z + b * img, code + b * img, code + b * img + img / 2, 1, H, W, sp_steps, stream);
        if (rc) return rc;
    }
    return VST_OK;
}

}  // extern "C"
