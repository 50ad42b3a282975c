"""Numpy restatements for per-frame strength maps (helpers of test_strength_frames_host.py / test_gpu_strength_frames.py).

``strength_frame`` is vst_strength_frame's arithmetic (include/vstnet.h), operation for operation in float32; ``rows_of`` is
vst_map_to_code's order.  ``box2`` is Pillow's ``Image.BOX`` 2 x 2 on 8-bit data (two rounded passes, horizontal first) and
``pil_resize_grey`` Pillow's 8-bit ``Image.BILINEAR`` resize of an "L" image: the arithmetic of tests/resize_ref.py with the
triangle filter of support 1.  Python floats are IEEE doubles and numpy float32 operations round once each, so these are the
numbers Pillow and the kernels compute.
"""
import math

import numpy as np

PRECISION_BITS = 22
F = np.float32


def triangle(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def ksize_of(in_size, out_size):
    return int(math.ceil(max(1.0, in_size / out_size))) * 2 + 1


def pil_coeffs_bilinear(in_size, out_size):
    """(ksize, bounds int32 [out,2], kk int32 [out,ksize]): precompute_coeffs + normalize_coeffs_8bpc for BILINEAR."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    ksize = ksize_of(in_size, out_size)
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws = [triangle((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = ws
    ints = np.where(kk < 0, -0.5 + kk * (1 << PRECISION_BITS), 0.5 + kk * (1 << PRECISION_BITS))
    return ksize, bounds, np.trunc(ints).astype(np.int32)


def _pass(img, out_size, axis):
    """One pass along `axis` (0 = vertical, 1 = horizontal) of a uint8 [H,W] image."""
    _, bounds, kk = pil_coeffs_bilinear(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for i in range(out_size):
        first, n = bounds[i]
        acc = np.tensordot(kk[i, :n].astype(np.int64), src[first:first + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize_grey(img, size_wh):
    """``np.asarray(Image.fromarray(img).resize(size_wh, Image.BILINEAR))`` for a uint8 [H,W] array."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    w, h = int(size_wh[0]), int(size_wh[1])
    if img.shape[1] != w:
        img = _pass(img, w, 1)
    if img.shape[0] != h:
        img = _pass(img, h, 0)
    return np.ascontiguousarray(img)


def box2(img):
    """``Image.fromarray(img).resize((W // 2, H // 2), Image.BOX)`` for a uint8 [H,W] array with even H, W."""
    a = img.astype(np.int32)
    h = (a[:, 0::2] + a[:, 1::2] + 1) >> 1
    return ((h[0::2] + h[1::2] + 1) >> 1).astype(np.uint8)


def strength_frame(matte, labels, table, sp):
    """vst_strength_frame's `dense`: float32 [cH,cW] from a uint8 [H,W] matte and / or label map and a float32 [256] table."""
    m = t = None
    if matte is not None:
        v = matte if sp == 2 else box2(matte)
        m = v.astype(F) / F(255)
    if labels is not None:
        tl = np.asarray(table, dtype=F)[labels]
        t = tl if sp == 2 else ((tl[0::2, 0::2] + tl[0::2, 1::2]) + (tl[1::2, 0::2] + tl[1::2, 1::2])) * F(0.25)
        assert t.dtype == F
    if m is None:
        return t
    return m if t is None else m * t


def rows_of(dense, H, W, sp):
    """vst_map_to_code in numpy: `dense` [cH,cW] in the packed code's row order (H, W = the FRAME's size)."""
    Hq, Wq = H // 4, W // 4
    per = 8 if sp == 2 else 2
    r = np.arange(2 * Hq * Wq * per)
    i, rr = r // (Hq * Wq * per), r % (Hq * Wq * per)
    cell, g = rr // per, rr % per
    h, w = cell // Wq, cell % Wq
    if sp == 2:
        return dense[4 * h + 2 * i + ((g >> 1) & 1), 4 * w + 2 * (g >> 2) + (g & 1)]
    return dense[2 * h + i, 2 * w + g]


def grey(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
