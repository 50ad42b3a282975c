"""The reference, the cases and the bounds for the deep resize (include/vstnet.h, "Deep resize").  The
arithmetic lives in vstnet_amd: resize.img_resize_float (numpy float64, no rounding anywhere) of yuv.yuv16_to_rgb_float.  This
module adds the shapes, the two bounds and the helpers the host and the GPU tests share.

The bounds.  A pass is out = M in with M's rows Pillow's normalised weights; bicubic rows have negative lobes, so an error e in a
pass's input grows to at most a e behind it, a = the pass's largest row sum of |w| (its gain; 1 <= a < 1.3).

  PILLOW (img_resize_float against utils.utils.img_resize, on the 0..255 scale, bytes drawn from 48..207 so that Pillow's clamp
  to 0..255 after each pass never fires): Pillow rounds to a byte once per pass - at most 0.5, amplified by the passes behind it -
  and rounds its coefficients to 22 bits - at most 2^-23 each, ksize of them on values up to 255, amplified likewise:
      B = sum_k (0.5 + 255 ksize_k 2^-23) prod_{j > k} a_j.

  KERNEL (vst_yuv16_img_resize_f32 against the float64 reference, on the 0..1 scale): the kernels accumulate in fp64 - errors
  of 1e-16, which do not count next to what follows - and round to fp32 once per store: the converted pixel (in LDS or, unfused,
  in memory; the same fp32 either way) and every pass's result.  A stored value v has |v| <= prod_{j <= k} a_j (the input lies
  in [0, 1]) and one rounding errs by at most 2^-24 |v| (half a spacing; the spacing is at most 2^-23 |v|), which the passes
  behind it amplify by prod_{j > k} a_j: every store contributes at most 2^-24 prod_k a_k, so
      T = (fp32 stores on the path) 2^-24 prod_k a_k,     stores = passes + 1.
  The final clamp to [0, 1] moves no value away from the clamped reference.  A few 1e-7; no measured constant."""
import numpy as np

from vstnet_amd.resize import coeffs_f64, float_passes, img_resize_float, img_resize_size  # noqa: F401
from vstnet_amd.yuv import DeepYuvSpec, rgb_to_yuv16_host, yuv16_to_rgb_float  # noqa: F401
from yuv16_ref import as_flat, random_planes, write_raw  # noqa: F401

# (source W, source H, max_size): what each exercises is in the tests' docstrings
SHAPES = [(97, 55, 64),         # -> 64x36: odd source, ceil chroma planes, both axes
          (42, 56, 64),         # -> 40x56: horizontal only, one step: the fused pass is also the last
          (40, 58, 64),         # -> 40x56: vertical only: the unfused entry
          (160, 140, 12),       # -> 12x10 -> 12x8: a shrink of 13.3 (ksize 55), two steps
          (301, 77, 150)]       # -> 150x38 -> 148x36: four passes, more than one column tile, a row-tile remainder
DOWN_SCALE = 4


def gains(size_wh, max_size):
    """[(a, ksize)] of the passes in order: a = the largest row sum of |w|"""
    out = []
    for _, n_in, n_out in float_passes(size_wh, max_size, DOWN_SCALE):
        ks, _, w = coeffs_f64(n_in, n_out)
        out.append((float(np.abs(w).sum(axis=1).max()), ks))
    return out


def pillow_bound(size_wh, max_size):
    """B of the module docstring, on the 0..255 scale"""
    g = gains(size_wh, max_size)
    return sum((0.5 + 255.0 * ks * 2.0 ** -23) * float(np.prod([a for a, _ in g[k + 1:]])) for k, (_, ks) in enumerate(g))


def kernel_tolerance(size_wh, max_size):
    """T of the module docstring, on the 0..1 scale"""
    g = gains(size_wh, max_size)
    return (len(g) + 1) * 2.0 ** -24 * float(np.prod([a for a, _ in g]))


def reference(flat, H, W, spec, max_size):
    """float64 [h, w, 3] in [0, 1]: what vst_yuv16_img_resize_f32 computes, without its roundings to fp32"""
    return np.clip(img_resize_float(yuv16_to_rgb_float(flat, H, W, spec), max_size, DOWN_SCALE), 0.0, 1.0)


def reference_frame(flat, H, W, spec, max_size, out_spec):
    """the flat bytes of a clip's stylised frame under --stub_stylise: the reference above as codes of out_spec"""
    return rgb_to_yuv16_host(reference(flat, H, W, spec, max_size), out_spec)


def twin_of(out_f32):
    """the u8 twin of a float output [..]: floor(255 double(v) + 0.5) of the stored fp32 values - an exact function of them"""
    return np.floor(255.0 * np.asarray(out_f32, np.float32).astype(np.float64) + 0.5).astype(np.uint8)
