"""Numpy restatement for per-frame style maps (helper of test_style_frames_host.py / test_gpu_style_frames*.py).

``style_frame`` is vst_style_frame's arithmetic (include/vstnet.h, "Style maps per frame"), operation for operation in float32;
the reduction to an artistic code's grid (``box2``), the packed rows' order (``rows_of``) and Pillow's 8-bit BILINEAR
(``pil_resize_grey``) are those of tests/strength_frames_ref.py.  numpy float32 operations round once each, so these are the
numbers the kernel and the host route (utils.utils.style_map_weights) compute.
"""
import numpy as np

from tests.strength_frames_ref import box2, pil_resize_grey, rows_of  # noqa: F401  (the tests take all three from here)

F = np.float32


def style_frame(planes, sp):
    """vst_style_frame's `dense` and whether it raises the flag: planes uint8 [P,H,W] -> (float32 [K,cH,cW], bool); P = 1 is
    the ramp between two styles (K = 2), P >= 2 one plane per style (K = P).  A code pixel at which every plane is 0 takes
    the first style alone."""
    planes = np.asarray(planes, dtype=np.uint8)
    assert planes.ndim == 3 and 1 <= planes.shape[0] <= 8
    u = planes if sp == 2 else np.stack([box2(p) for p in planes])
    if u.shape[0] == 1:
        t = u[0].astype(F) / F(255)
        return np.stack([F(1) - t, t]), False
    total = u.astype(np.int32).sum(axis=0)
    zero = total == 0
    tf = np.where(zero, 1, total).astype(F)               # (the flagged pixels are overwritten below: no 0 / 0 here)
    w = np.stack([p.astype(F) / tf for p in u])
    assert w.dtype == F
    w[0][zero] = F(1)
    w[1:, zero] = F(0)
    return w, bool(zero.any())


def planes_of(P, H, W, seed, lo=0):
    """random uint8 [P,H,W] planes; lo = 1 keeps every pixel's sum above 0"""
    return np.random.default_rng(seed).integers(lo, 256, (P, H, W), dtype=np.uint8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
