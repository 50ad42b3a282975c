"""ctypes binding of libvstnet_hip.so (C ABI declared in include/vstnet.h) and its in-tree build.

There is deliberately no fallback: if the shared library is missing or a call returns a non-zero
status, a ``VstError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("VSTNET_HIP_LIB") or os.path.join(PKG_DIR, "libvstnet_hip.so")   # override: A/B builds
RESOURCES_PATH = os.path.join(PKG_DIR, "libvstnet_hip.resources.txt")    # per-kernel VGPRs / LDS / scratch of the last build
SOURCES = sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.hip")))
HEADERS = sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.h"))) + [os.path.join(REPO_DIR, "include", "vstnet.h")]

NUM_BLOCKS = 32
PREC_BF16X3 = 0
PREC_FP32 = 1
PREC_F16X2 = 2
PREC_F16X2H = 3

# every symbol include/vstnet.h declares
EXPORTS = [
    "vst_version", "vst_error_string", "vst_conv_packed_bytes", "vst_pack_conv", "vst_pack_input",
    "vst_unpack_output", "vst_pack_input_u8", "vst_unpack_output_u8", "vst_revnet_forward_u8", "vst_revnet_inverse_u8",
    "vst_spread", "vst_gather", "vst_block_tmp_bytes", "vst_block_apply",
    "vst_pass_workspace_bytes", "vst_revnet_forward", "vst_revnet_inverse",
    "vst_cwct_stats_workspace_bytes", "vst_cwct_stats", "vst_cwct_factor", "vst_cwct_apply", "vst_cwct_apply_prec",
    "vst_cwct_prefactor", "vst_label_plan", "vst_cwct_labels_workspace_bytes", "vst_cwct_stats_labels",
    "vst_cwct_factor_labels", "vst_cwct_apply_labels", "vst_profile_begin", "vst_profile_end", "vst_profile_end_table", "vst_lab_luminance",
    "vst_revnet_encode", "vst_revnet_encode_u8", "vst_revnet_decode", "vst_revnet_decode_u8", "vst_code_to_z", "vst_z_to_code",
    "vst_cwct_stats_code_workspace_bytes", "vst_cwct_stats_code", "vst_cwct_apply_code",
    "vst_mask_to_code", "vst_cwct_stats_labels_code_workspace_bytes", "vst_cwct_stats_labels_code", "vst_cwct_apply_labels_code",
    "vst_revnet_decode_labels", "vst_revnet_decode_labels_u8", "vst_pass_sub_batch",
    "vst_normalize_block", "vst_range_flags", "vst_range_flags_async",
    "vst_cwct_stats_f64_workspace_bytes", "vst_cwct_stats_f64", "vst_cwct_factor_f64_workspace_bytes", "vst_cwct_factor_f64",
    "vst_cwct_apply_f64",
    "vst_generic_conv", "vst_generic_squeeze", "vst_generic_unsqueeze", "vst_generic_copy_channels", "vst_generic_zero",
    "vst_set_option", "vst_get_option",
    "vst_cwct_stats_n_workspace_bytes", "vst_cwct_stats_n", "vst_cwct_factor_n_workspace_bytes", "vst_cwct_factor_n",
    "vst_cwct_prefactor_n", "vst_cwct_apply_n", "vst_cwct_stats_n_f64_workspace_bytes", "vst_cwct_stats_n_f64",
    "vst_cwct_factor_n_f64_workspace_bytes", "vst_cwct_factor_n_f64", "vst_cwct_apply_n_f64",
    "vst_max_frame_pixels", "vst_cwct_stats_code_rect", "vst_cwct_stats_labels_code_rect",
    "vst_colors_to_labels", "vst_label_hist", "vst_mask_prepare", "vst_remap_lut", "vst_apply_lut", "vst_label_plan_hist",
    "vst_cwct_factor_labels_keyed",
    "vst_label_plan_hists", "vst_cwct_factor_labels_mix", "vst_cwct_prefactor_labels",
    "vst_resize_coeffs_u8", "vst_resize_u8", "vst_resize_coeffs_f32", "vst_resize_f32", "vst_resize_f32_to_u8",
    "vst_lab_luminance_u8", "vst_lab_luminance_u8_f32",
    "vst_seg_create", "vst_seg_tensor_count", "vst_seg_tensor_info", "vst_seg_load_tensor", "vst_seg_run_u8", "vst_seg_logits",
    "vst_seg_shape", "vst_seg_destroy", "vst_seg_run_scaled_u8", "vst_seg_labels_from_logits",
    "vst_seg_mix_logits",
    "vst_seg_gemm", "vst_seg_layernorm", "vst_seg_attention", "vst_seg_dwconv_gelu", "vst_seg_im2col", "vst_seg_gather_rgb",
    "vst_seg_head_sum",
    "vst_map_to_code", "vst_cwct_apply_code_blend", "vst_cwct_apply_labels_code_blend", "vst_revnet_decode_blend",
    "vst_revnet_decode_blend_u8", "vst_revnet_decode_labels_blend", "vst_revnet_decode_labels_blend_u8", "vst_cwct_blend",
    "vst_strength_frame", "vst_resize_coeffs_u8_bilinear", "vst_resize_grey_u8",
    "vst_cwct_apply_code_mix", "vst_revnet_decode_mix", "vst_revnet_decode_mix_u8", "vst_cwct_mix_acc",
    "vst_cwct_stats_pool", "vst_cwct_stats_pool_keyed",
    "vst_yuv_to_rgb_u8", "vst_rgb_to_yuv_u8",
    "vst_yuv16_to_rgb_f32", "vst_rgb_f32_to_yuv16",
    "vst_resize_coeffs_f64", "vst_yuv16_img_resize_workspace_bytes", "vst_yuv16_img_resize_f32",
    "vst_guided_workspace_bytes", "vst_guided_fit", "vst_guided_apply_u8", "vst_guided_apply_f32",
    "vst_matting_workspace_bytes", "vst_matting_loss_f32", "vst_matting_loss_u8",
    "vst_warp_u8", "vst_warp_f32", "vst_temporal_workspace_bytes", "vst_temporal_l1_u8", "vst_temporal_l1_f32",
    "vst_fake_flow_workspace_bytes", "vst_fake_flow",
    "vst_flow_workspace_bytes", "vst_flow_lk_u8", "vst_flow_consistency", "vst_temporal_l1_masked_u8",
    "vst_style_frame",
    "vst_stabilise_u8",
    "vst_vgg_create", "vst_vgg_load_tensor", "vst_vgg_workspace_bytes", "vst_vgg_features_u8", "vst_vgg_features_f32",
    "vst_vgg_destroy", "vst_vgg_input_u8", "vst_vgg_input_f32", "vst_vgg_conv3x3_relu", "vst_vgg_maxpool2",
    "vst_vgg_mean_std_workspace_bytes", "vst_vgg_mean_std", "vst_vgg_mse_f64", "vst_vgg_style_loss",
]
VGG_RECORD_DOUBLES = 1920    # vstnet.h VST_VGG_RECORD_DOUBLES
VGG_MSE_WS_BYTES = 8192      # vstnet.h VST_VGG_MSE_WS_BYTES
FLOW_MAX_LEVELS, FLOW_MAX_ITERS, FLOW_MAX_RADIUS = 8, 16, 7      # vstnet.h VST_FLOW_MAX_*
FAKE_FLOW_MAX_GRID = 1024    # vstnet.h VST_FAKE_FLOW_MAX_GRID
MATTING_MAX_RADIUS = 3       # vstnet.h VST_MATTING_MAX_RADIUS
GUIDED_MAX_RADIUS = 8        # vstnet.h VST_GUIDED_MAX_RADIUS
MAX_STYLES = 8               # csrc/common.h CWCT_MAX_STYLES: styles one factor launch mixes
SEG_MIX_MAX = 8              # vstnet.h VST_SEG_MIX_MAX: frames one vst_seg_mix_logits launch mixes
KERNEL_SEG_MIX = 9           # vstnet.h VST_KERNEL_SEG_MIX
STATS_POOL_MAX = 8           # vstnet.h VST_STATS_POOL_MAX: frames one vst_cwct_stats_pool launch pools
KERNEL_CWCT_POOL = 10        # vstnet.h VST_KERNEL_CWCT_POOL
MASK_OVERFLOW = 1            # vstnet.h VST_MASK_*: bits of a frame's mask flag word
MASK_OUT_OF_TABLE = 2
LABEL_PLAN_BYTES = 2344
OPT_STAGE3_LEAN = 1
OPT_STAGE3_WIDE = 3
OPT_STAGE1_FOLD = 4
OPT_OUT_RGB = 5
YUV_444, YUV_420_CENTRE, YUV_420_LEFT = 0, 1, 2     # vstnet.h VST_YUV_*: layout, matrix, range
YUV_422 = 3                                         # (the high-bit-depth edge only: the _u8 calls refuse it)
YUV_BT601, YUV_BT709 = 0, 1
YUV_LIMITED, YUV_FULL = 0, 1
RANGE_SATURATED = 1
RANGE_WEIGHT = 2


PRECISIONS = {"bf16x3": PREC_BF16X3, "fp32": PREC_FP32, "f16x2": PREC_F16X2, "f16x2h": PREC_F16X2H}


def default_precision() -> str:
    """bf16x3: the fp32-class arithmetic (3e-6 of the reference).  The fp16 modes are opt-in (per module, or VST_PRECISION):
    they round the weights to 11 bits, which DESIGN.md section 3 prices at 1.5e-4 on well-conditioned codes and at more than
    the 1e-3 budget on ill-conditioned ones (tests/test_gpu_robust.py)."""
    p = os.environ.get("VST_PRECISION", "bf16x3")
    if p not in PRECISIONS:
        raise ValueError(f"VST_PRECISION must be one of {sorted(PRECISIONS)}")
    return p


class VstError(RuntimeError):
    pass


class ConvWeights(C.Structure):
    _fields_ = [("packed", C.c_void_p), ("bias", C.c_void_p)]


class BlockWeights(C.Structure):
    _fields_ = [("conv", ConvWeights * 3)]


class NetWeights(C.Structure):
    _fields_ = [("blocks", BlockWeights * NUM_BLOCKS)]


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into vstnet_amd/libvstnet_hip.so (cross-compiles without a GPU)."""
    newest_src = max(os.path.getmtime(p) for p in SOURCES + HEADERS)
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest_src:
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # host code with hidden default visibility: the shared library exports exactly what include/vstnet.h declares
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-fPIC", "-shared", "-std=c++17", "-Xarch_host", "-fvisibility=hidden",
           "-I", os.path.join(REPO_DIR, "include"), "-o", LIB_PATH] + SOURCES
    cmd[1:1] = ["-Rpass-analysis=kernel-resource-usage", "-fno-caret-diagnostics"]   # per-kernel registers / LDS / scratch as remarks
    if verbose:
        print(" ".join(cmd))
    p = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    remarks = [ln.split("remark:", 1)[1].split("[-Rpass")[0].strip() for ln in p.stderr.splitlines() if "remark:" in ln]
    other = "\n".join(ln for ln in p.stderr.splitlines() if "remark:" not in ln and "kernel-resource-usage" not in ln)
    if p.returncode != 0:
        raise subprocess.CalledProcessError(p.returncode, cmd, stderr=other)
    if other.strip():
        print(other)
    # no kernel of this library may spill: a private segment means scratch traffic in a hot loop (DESIGN.md section 6 has the
    # story of a 20 % regression from one).  The table is kept next to the library for inspection.
    table, name = [], None
    for r in remarks:
        if r.startswith("Function Name:"):
            name = r.split(":", 1)[1].strip()
        elif name and (r.startswith("VGPRs:") or r.startswith("ScratchSize") or r.startswith("LDS Size") or r.startswith("Occupancy")):
            table.append(f"{name}\t{r}")
    with open(RESOURCES_PATH, "w") as f:
        f.write("\n".join(table) + "\n")
    spills = [t for t in table if "ScratchSize" in t and not t.rstrip().endswith(": 0")]
    if spills:
        os.remove(LIB_PATH)
        raise RuntimeError("kernels with a private segment (register spills):\n" + "\n".join(spills))
    return LIB_PATH


RUNNER_SRC = os.path.join(REPO_DIR, "tools", "vst_run.cpp")
RUNNER_BIN = os.path.join(REPO_DIR, "tools", "vst_run")


def build_runner(force: bool = False) -> str:
    """Compile the native (no Python / torch) host runner against the shared library."""
    if not force and os.path.exists(RUNNER_BIN) and os.path.getmtime(RUNNER_BIN) >= max(os.path.getmtime(RUNNER_SRC),
                                                                                       os.path.getmtime(LIB_PATH)):
        return RUNNER_BIN
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(REPO_DIR, "include"), RUNNER_SRC,
           "-L", PKG_DIR, "-lvstnet_hip", "-Wl,-rpath," + PKG_DIR, "-Wl,-rpath,$ORIGIN/../vstnet_amd", "-o", RUNNER_BIN]
    subprocess.run(cmd, check=True)
    return RUNNER_BIN


_lib = None


def lib() -> C.CDLL:
    """Load the library (never builds implicitly on a box without hipcc; raises if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VstError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the HIP path)")
    L = C.CDLL(LIB_PATH)
    vp, i, f, sz, lg = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_long
    sig = {
        "vst_version": (i, []),
        "vst_error_string": (C.c_char_p, [i]),
        "vst_conv_packed_bytes": (sz, [i, i]),
        "vst_pack_conv": (i, [vp, i, i, vp, vp]),
        "vst_normalize_block": (i, [vp, vp, vp, vp, vp, i, i, i, vp, vp]),
        "vst_range_flags": (i, [C.POINTER(C.c_uint), i]),
        "vst_range_flags_async": (i, [vp, vp]),
        "vst_pack_input": (i, [vp, vp, vp, i, i, i, i, vp]),
        "vst_unpack_output": (i, [vp, vp, i, i, i, i, vp]),
        "vst_pack_input_u8": (i, [vp, vp, vp, i, i, i, vp]),
        "vst_unpack_output_u8": (i, [vp, vp, i, i, i, vp]),
        "vst_lab_luminance": (i, [vp, vp, vp, i, i, i, vp]),
        "vst_lab_luminance_u8": (i, [vp, vp, vp, i, i, i, vp]),
        "vst_lab_luminance_u8_f32": (i, [vp, vp, vp, i, i, i, vp]),
        "vst_revnet_forward_u8": (i, [C.POINTER(NetWeights), vp, vp, vp, i, i, i, i, i, vp]),
        "vst_revnet_inverse_u8": (i, [C.POINTER(NetWeights), vp, vp, vp, i, i, i, i, i, vp]),
        "vst_spread": (i, [vp, vp, vp, i, i, i, i, vp]),
        "vst_gather": (i, [vp, vp, vp, i, i, i, i, vp]),
        "vst_block_tmp_bytes": (sz, [i, i, i]),
        "vst_block_apply": (i, [C.POINTER(BlockWeights), i, i, i, i, vp, vp, vp, i, i, i, vp]),
        "vst_pass_workspace_bytes": (sz, [i, i, i]),
        "vst_pass_sub_batch": (i, [i, i, i]),
        "vst_revnet_forward": (i, [C.POINTER(NetWeights), vp, vp, vp, i, i, i, i, i, i, vp]),
        "vst_revnet_inverse": (i, [C.POINTER(NetWeights), vp, vp, vp, i, i, i, i, i, i, vp]),
        "vst_cwct_stats_workspace_bytes": (sz, [i, lg]),
        "vst_cwct_stats": (i, [vp, i, lg, vp, i, vp, vp, vp]),
        "vst_cwct_factor": (i, [vp, C.POINTER(vp), C.POINTER(f), i, f, f, i, vp, vp, vp]),
        "vst_cwct_apply": (i, [vp, vp, i, lg, vp, vp, i, vp]),
        "vst_cwct_apply_prec": (i, [vp, vp, i, lg, vp, vp, i, i, vp]),
        "vst_cwct_prefactor": (i, [vp, i, f, vp, vp, vp]),
        "vst_cwct_stats_f64_workspace_bytes": (sz, [i, lg]),
        "vst_cwct_stats_f64": (i, [vp, i, lg, vp, i, vp, vp, vp]),
        "vst_cwct_factor_f64_workspace_bytes": (sz, [i]),
        "vst_cwct_factor_f64": (i, [vp, C.POINTER(vp), C.POINTER(f), i, f, f, i, vp, vp, vp, vp]),
        "vst_cwct_apply_f64": (i, [vp, vp, i, lg, vp, vp, i, vp]),
        "vst_cwct_stats_n_workspace_bytes": (sz, [i, lg]),
        "vst_cwct_stats_n": (i, [vp, i, lg, vp, i, vp, vp, sz, vp]),
        "vst_cwct_factor_n_workspace_bytes": (sz, [i]),
        "vst_cwct_factor_n": (i, [vp, C.POINTER(vp), C.POINTER(f), i, f, f, i, vp, vp, vp, sz, vp]),
        "vst_cwct_prefactor_n": (i, [vp, i, f, vp, vp, vp, sz, vp]),
        "vst_cwct_apply_n": (i, [vp, vp, i, lg, vp, vp, i, vp]),
        "vst_cwct_stats_n_f64_workspace_bytes": (sz, [i, lg]),
        "vst_cwct_stats_n_f64": (i, [vp, i, lg, vp, i, vp, vp, sz, vp]),
        "vst_cwct_factor_n_f64_workspace_bytes": (sz, [i]),
        "vst_cwct_factor_n_f64": (i, [vp, C.POINTER(vp), C.POINTER(f), i, f, f, i, vp, vp, vp, sz, vp]),
        "vst_cwct_apply_n_f64": (i, [vp, vp, i, lg, vp, vp, i, vp]),
        "vst_generic_conv": (i, [vp, vp, vp, vp, f, i, vp, i, i, i, i, i, i, i, vp]),
        "vst_generic_squeeze": (i, [vp, vp, i, i, i, i, vp]),
        "vst_generic_unsqueeze": (i, [vp, vp, i, i, i, i, vp]),
        "vst_generic_copy_channels": (i, [vp, vp, i, i, i, i, lg, i, i, vp]),
        "vst_generic_zero": (i, [vp, sz, vp]),
        "vst_label_plan": (i, [vp, lg, vp, lg, vp, vp]),
        "vst_cwct_labels_workspace_bytes": (sz, [i, lg]),
        "vst_cwct_stats_labels": (i, [vp, i, lg, vp, vp, i, vp, vp, vp]),
        "vst_cwct_factor_labels": (i, [vp, vp, vp, i, f, i, vp, vp, vp]),
        "vst_cwct_apply_labels": (i, [vp, vp, i, lg, vp, vp, vp, i, i, vp]),
        "vst_revnet_encode": (i, [C.POINTER(NetWeights), vp, vp, vp, i, i, i, i, i, vp]),
        "vst_revnet_encode_u8": (i, [C.POINTER(NetWeights), vp, vp, vp, i, i, i, i, vp]),
        "vst_revnet_decode": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, i, i, i, i, i, i, vp]),
        "vst_revnet_decode_u8": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, i, i, i, i, i, vp]),
        "vst_code_to_z": (i, [vp, vp, i, i, i, i, vp]),
        "vst_z_to_code": (i, [vp, vp, i, i, i, i, vp]),
        "vst_cwct_stats_code_workspace_bytes": (sz, [i, i, i]),
        "vst_cwct_stats_code": (i, [vp, i, i, i, vp, vp, vp]),
        "vst_cwct_apply_code": (i, [vp, vp, i, i, i, vp, vp]),
        "vst_mask_to_code": (i, [vp, vp, i, i, vp]),
        "vst_cwct_stats_labels_code_workspace_bytes": (sz, [i, i]),
        "vst_cwct_stats_labels_code": (i, [vp, i, i, vp, vp, i, vp, vp, vp]),
        "vst_cwct_apply_labels_code": (i, [vp, vp, i, i, vp, vp, vp, i, vp]),
        "vst_revnet_decode_labels": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, i, vp, vp, i, i, i, i, vp]),
        "vst_revnet_decode_labels_u8": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, i, vp, vp, i, i, i, vp]),
        "vst_map_to_code": (i, [vp, vp, i, i, i, vp]),
        "vst_cwct_apply_code_blend": (i, [vp, vp, i, i, i, vp, vp, vp]),
        "vst_cwct_apply_labels_code_blend": (i, [vp, vp, i, i, vp, vp, vp, i, vp, vp]),
        "vst_revnet_decode_blend": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]),
        "vst_revnet_decode_blend_u8": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, vp, i, i, i, i, i, vp]),
        "vst_revnet_decode_labels_blend": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, i, vp, vp, vp, i, i, i, i, vp]),
        "vst_revnet_decode_labels_blend_u8": (i, [C.POINTER(NetWeights), vp, vp, vp, vp, i, vp, vp, vp, i, i, i, vp]),
        "vst_cwct_blend": (i, [vp, vp, vp, vp, i, lg, vp]),
        "vst_strength_frame": (i, [vp, vp, vp, vp, vp, i, i, i, vp]),
        "vst_style_frame": (i, [vp, i, vp, vp, vp, i, i, i, vp]),
        "vst_cwct_apply_code_mix": (i, [vp, vp, i, i, i, vp, i, vp, vp, vp]),
        "vst_revnet_decode_mix": (i, [C.POINTER(NetWeights), vp, vp, i, vp, vp, vp, vp, i, i, i, i, i, i, vp]),
        "vst_revnet_decode_mix_u8": (i, [C.POINTER(NetWeights), vp, vp, i, vp, vp, vp, vp, i, i, i, i, i, vp]),
        "vst_cwct_mix_acc": (i, [vp, vp, vp, i, lg, i, vp]),
        "vst_resize_coeffs_u8_bilinear": (i, [i, i, C.POINTER(i), vp, vp]),
        "vst_resize_grey_u8": (i, [vp, i, i, vp, i, i, vp, vp, vp]),
        "vst_max_frame_pixels": (C.c_int64, []),
        "vst_cwct_stats_code_rect": (i, [vp, i, i, i, i, i, i, i, vp, vp, vp]),
        "vst_cwct_stats_labels_code_rect": (i, [vp, i, i, i, i, i, i, vp, vp, i, vp, vp, vp]),
        "vst_colors_to_labels": (i, [vp, vp, lg, vp]),
        "vst_label_hist": (i, [vp, lg, vp, vp]),
        "vst_mask_prepare": (i, [vp, i, i, i, vp, vp, vp]),
        "vst_remap_lut": (i, [vp, vp, vp, i, i, i, vp, vp, vp, vp]),
        "vst_apply_lut": (i, [vp, vp, vp, lg, vp]),
        "vst_label_plan_hist": (i, [vp, vp, vp, i, vp, vp, vp]),
        "vst_cwct_factor_labels_keyed": (i, [vp, vp, vp, vp, i, f, i, vp, vp, vp]),
        "vst_label_plan_hists": (i, [vp, vp, C.POINTER(vp), i, i, vp, vp, vp]),
        "vst_cwct_factor_labels_mix": (i, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(f), i, f, vp, i, f, i, vp, vp, vp]),
        "vst_cwct_prefactor_labels": (i, [vp, vp, i, i, f, vp, vp, vp]),
        "vst_resize_coeffs_u8": (i, [i, i, C.POINTER(i), vp, vp]),
        "vst_resize_u8": (i, [vp, i, i, vp, i, i, vp, vp, vp]),
        "vst_resize_coeffs_f32": (i, [i, i, C.POINTER(i), vp, vp]),
        "vst_resize_f32": (i, [vp, i, i, i, vp, i, i, vp, vp, vp]),
        "vst_resize_f32_to_u8": (i, [vp, i, i, i, vp, i, i, vp, vp, vp]),
        "vst_seg_create": (i, [C.POINTER(i), i, C.POINTER(vp)]),
        "vst_seg_tensor_count": (i, [vp]),
        "vst_seg_tensor_info": (i, [vp, i, C.POINTER(C.c_char_p), C.POINTER(sz)]),
        "vst_seg_load_tensor": (i, [vp, C.c_char_p, vp, sz]),
        "vst_seg_run_u8": (i, [vp, vp, i, i, i, vp, vp]),
        "vst_seg_run_scaled_u8": (i, [vp, vp, i, i, i, i, i, vp, vp]),
        "vst_seg_labels_from_logits": (i, [vp, i, i, i, i, i, vp, vp]),
        "vst_seg_logits": (i, [vp, vp, i, i, i, vp, vp, vp, vp, vp, vp]),
        "vst_seg_shape": (i, [i, i, C.POINTER(i)]),
        "vst_seg_mix_logits": (i, [C.POINTER(vp), C.POINTER(f), i, sz, vp, vp]),
        "vst_cwct_stats_pool": (i, [C.POINTER(vp), C.POINTER(C.c_double), i, i, i, C.c_double, vp, vp, vp]),
        "vst_cwct_stats_pool_keyed": (i, [C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_double), i, i, i, C.c_double, vp, vp, vp]),
        "vst_seg_destroy": (i, [vp]),
        "vst_seg_gemm": (i, [vp, vp, vp, vp, vp, i, i, i, vp]),
        "vst_seg_layernorm": (i, [vp, vp, vp, vp, i, i, f, vp]),
        "vst_seg_attention": (i, [vp, vp, vp, i, i, i, f, vp]),
        "vst_seg_dwconv_gelu": (i, [vp, vp, vp, vp, i, i, i, vp]),
        "vst_seg_im2col": (i, [vp, i, i, i, i, i, i, vp, vp]),
        "vst_seg_gather_rgb": (i, [vp, i, i, i, vp, vp]),
        "vst_seg_head_sum": (i, [vp, vp, vp, vp, C.POINTER(i), i, vp, vp]),
        "vst_yuv_to_rgb_u8": (i, [vp, vp, vp, i, i, i, i, i, vp, vp]),
        "vst_rgb_to_yuv_u8": (i, [vp, i, i, i, i, i, vp, vp, vp, vp]),
        "vst_yuv16_to_rgb_f32": (i, [vp, vp, vp, i, i, i, i, i, i, vp, vp, vp]),
        "vst_rgb_f32_to_yuv16": (i, [vp, i, i, i, i, i, i, vp, vp, vp, vp]),
        "vst_resize_coeffs_f64": (i, [i, i, C.POINTER(i), vp, vp]),
        "vst_yuv16_img_resize_workspace_bytes": (i, [i, i, i, C.POINTER(i), C.POINTER(sz)]),
        "vst_yuv16_img_resize_f32": (i, [vp, vp, vp, i, i, i, i, i, i, i, C.POINTER(i), vp, vp, vp, vp, vp]),
        "vst_guided_workspace_bytes": (i, [i, i, i, C.POINTER(sz)]),
        "vst_guided_fit": (i, [vp, vp, i, i, i, C.c_double, vp, vp, vp]),
        "vst_guided_apply_u8": (i, [vp, i, i, vp, i, i, vp, vp]),
        "vst_guided_apply_f32": (i, [vp, i, i, vp, i, i, vp, vp]),
        "vst_matting_workspace_bytes": (i, [i, i, i, C.POINTER(sz)]),
        "vst_matting_loss_f32": (i, [vp, vp, i, i, i, C.c_double, vp, vp, vp, vp]),
        "vst_matting_loss_u8": (i, [vp, vp, i, i, i, C.c_double, vp, vp, vp, vp]),
        "vst_warp_u8": (i, [vp, vp, vp, vp, i, i, vp]),
        "vst_warp_f32": (i, [vp, vp, vp, vp, i, i, vp]),
        "vst_temporal_workspace_bytes": (i, [i, i, C.POINTER(sz)]),
        "vst_temporal_l1_u8": (i, [vp, vp, vp, i, i, vp, vp, vp, vp]),
        "vst_temporal_l1_f32": (i, [vp, vp, vp, i, i, vp, vp, vp, vp]),
        "vst_fake_flow_workspace_bytes": (i, [i, i, i, i, i, C.POINTER(sz)]),
        "vst_fake_flow": (i, [vp, i, i, C.c_double, C.c_double, i, vp, i, i, vp, vp]),
        "vst_flow_workspace_bytes": (i, [i, i, i, C.POINTER(sz)]),
        "vst_flow_lk_u8": (i, [vp, vp, i, i, i, i, i, C.c_double, vp, vp, vp]),
        "vst_flow_consistency": (i, [vp, vp, i, i, vp, vp]),
        "vst_temporal_l1_masked_u8": (i, [vp, vp, vp, vp, i, i, vp, vp, vp, vp]),
        "vst_stabilise_u8": (i, [vp, vp, vp, vp, vp, vp, i, i, C.c_double, C.c_double, C.c_double, vp, vp]),
        "vst_vgg_create": (i, [C.POINTER(vp)]),
        "vst_vgg_load_tensor": (i, [vp, C.c_char_p, vp, sz]),
        "vst_vgg_workspace_bytes": (i, [i, i, C.POINTER(sz)]),
        "vst_vgg_features_u8": (i, [vp, vp, i, i, vp, vp, vp, sz, vp]),
        "vst_vgg_features_f32": (i, [vp, vp, i, i, vp, vp, vp, sz, vp]),
        "vst_vgg_destroy": (i, [vp]),
        "vst_vgg_input_u8": (i, [vp, vp, vp, vp, i, i, vp]),
        "vst_vgg_input_f32": (i, [vp, vp, vp, vp, i, i, vp]),
        "vst_vgg_conv3x3_relu": (i, [vp, vp, vp, vp, i, i, i, i, vp]),
        "vst_vgg_maxpool2": (i, [vp, vp, i, i, i, vp]),
        "vst_vgg_mean_std_workspace_bytes": (i, [i, i, C.POINTER(sz)]),
        "vst_vgg_mean_std": (i, [vp, i, i, C.c_double, vp, vp, sz, vp]),
        "vst_vgg_mse_f64": (i, [vp, vp, sz, vp, vp, vp]),
        "vst_vgg_style_loss": (i, [vp, vp, vp, vp]),
        "vst_set_option": (i, [i, i]),
        "vst_get_option": (i, [i]),
        "vst_profile_begin": (i, [i, i]),
        "vst_profile_end": (i, [C.POINTER(C.c_double), C.POINTER(i)]),
        "vst_profile_end_table": (i, [C.POINTER(i), C.POINTER(C.c_double), C.POINTER(i), i, C.POINTER(i)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


KERNEL_ALL = -1
MISC_KERNELS = {1: "pack_input", 2: "unpack_output", 3: "spread", 4: "gather", 5: "cwct_stats", 6: "cwct_factor",
                7: "cwct_apply", 8: "presplit", 9: "seg_mix", 10: "cwct_pool"}


def profile_table(run, max_records: int = 4096):
    """HIP-event time of every hooked launch that ``run()`` makes: {kernel id: (total ms, launches)}."""
    L = lib()
    check(L.vst_profile_begin(KERNEL_ALL, max_records), "vst_profile_begin")
    try:
        run()
    finally:
        ids, ms, cnt, n = (C.c_int * 64)(), (C.c_double * 64)(), (C.c_int * 64)(), C.c_int(0)
        check(L.vst_profile_end_table(ids, ms, cnt, 64, C.byref(n)), "vst_profile_end_table")
    return {ids[k]: (ms[k], cnt[k]) for k in range(n.value)}


def set_option(option: int, value: int) -> None:
    """Process-wide tuning option of include/vstnet.h (VST_OPT_*)."""
    check(lib().vst_set_option(option, int(value)), "vst_set_option")


def get_option(option: int) -> int:
    v = lib().vst_get_option(option)
    if v < 0:
        check(v, "vst_get_option")
    return v


def kernel_id(cin: int, cout: int, stride: int) -> int:
    """VST_KERNEL_ID of include/vstnet.h."""
    return (cin << 16) | (cout << 4) | stride


def range_flags(reset: bool = False) -> int:
    """fp16 range flags raised on the current device since the last reset (vstnet.h: VST_RANGE_*).  Synchronises the device."""
    v = C.c_uint(0)
    check(lib().vst_range_flags(C.byref(v), 1 if reset else 0), "vst_range_flags")
    return int(v.value)


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().vst_error_string(rc).decode()
        raise VstError(f"{what} failed with status {rc}: {msg}")
