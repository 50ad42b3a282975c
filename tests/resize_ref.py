"""Numpy restatements of the two resampling contracts of csrc/resize.hip (helpers of test_resize_host.py / test_gpu_resize.py).

``pil_resize`` is Pillow's 8-bit bicubic ``Image.resize`` stated as arithmetic: coefficients in double (support
2 * max(1, in/out), a = -0.5, normalised by their sum), rounded to 22-bit fixed point, each pass
``clip8((2^21 + sum px * k) >> 22)``, horizontal pass first with a uint8 intermediate, a pass whose size does not change
skipped.  ``aa_weights_f64`` is the antialiased bicubic weight formula of ``F.interpolate(..., antialias=True)`` in float64.
Python floats are IEEE doubles and nothing here is contracted into an fma, so these are the integers Pillow computes.
"""
import math

import numpy as np

PRECISION_BITS = 22


def cubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize_of(in_size, out_size):
    return int(math.ceil(2.0 * max(1.0, in_size / out_size))) * 2 + 1


def _rows(in_size, out_size, divide):
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    ksize = ksize_of(in_size, out_size)
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws = []
        ww = 0.0
        for x in range(xmax):
            t = x + xmin - center + 0.5
            w = cubic(t / filterscale if divide else t * ss)
            ws.append(w)
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = ws
    return ksize, bounds, kk


def pil_coeffs(in_size, out_size):
    """(ksize, bounds int32 [out,2], kk int32 [out,ksize]): precompute_coeffs + normalize_coeffs_8bpc for BICUBIC."""
    ksize, bounds, kk = _rows(in_size, out_size, False)
    ints = np.where(kk < 0, -0.5 + kk * (1 << PRECISION_BITS), 0.5 + kk * (1 << PRECISION_BITS))
    return ksize, bounds, np.trunc(ints).astype(np.int32)


def aa_weights_f64(in_size, out_size):
    """(ksize, bounds, w float64 [out,ksize]) of the antialiased bicubic resize, align_corners=False."""
    return _rows(in_size, out_size, True)


def _pass(img, out_size, axis):
    """One pass along `axis` (0 = vertical, 1 = horizontal) of a uint8 [H,W,C] image."""
    in_size = img.shape[axis]
    _, bounds, kk = pil_coeffs(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for i in range(out_size):
        first, n = bounds[i]
        acc = np.tensordot(kk[i, :n].astype(np.int64), src[first:first + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31          # Pillow's (and the kernel's) int32 accumulator is enough
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize(img, size_wh):
    """``np.asarray(Image.fromarray(img).resize(size_wh, Image.BICUBIC))`` for a uint8 [H,W,3] array."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    w, h = int(size_wh[0]), int(size_wh[1])
    if img.shape[1] != w:
        img = _pass(img, w, 1)
    if img.shape[0] != h:
        img = _pass(img, h, 0)
    return np.ascontiguousarray(img)


def frame(h, w, seed, smooth=False):
    """A seeded uint8 [h,w,3] test frame: random bytes (exercises clipping) or a smooth gradient (the rounding boundary)."""
    if not smooth:
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = seed * 0.37
    r = 127.5 + 127.5 * np.sin(x / w * 5.1 + y / h * 2.3 + ph)
    g = 255.0 * (x / max(w - 1, 1)) * (y / max(h - 1, 1))
    b = 127.5 + 100.0 * np.cos(y / h * 7.0 - x / w * 1.7 + ph) + 20.0 * np.sin(x * 0.05)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
