"""Frame resampling on the device (csrc/resize.hip): the resizes around the stylisation of a video frame.

Input side: ``utils.utils.img_resize`` (two PIL bicubic resizes per frame, video_transfer.py:161 of the reference) as
``img_resize_device`` on a uint8 HWC device tensor - the same size rule, the same integers, so the same bytes.  Output side:
``F.interpolate(bicubic, antialias=True)`` to the writer size followed by ``mul(255).clamp(0, 255).byte()`` and the HWC
permute (video_transfer.py:210-212) as ``resize_to_u8``, with the weights built in double.

Coefficient tables are built on the host by the library (vst_resize_coeffs_*), once per (in, out) pair, and kept on the
device; every call is queued on the current stream (or the one given) and never synchronises.  There is no CPU fallback here:
a shape the kernels do not take raises ``VstError`` (``device_supported`` tells beforehand).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

MAX_SHRINK = 16              # vstnet.h VST_RESIZE_MAX_SHRINK


# ------------------------------------------------------------------------------------------------ size arithmetic (pure Python)
def img_resize_steps(size_wh, max_size, down_scale=None):
    """The target sizes (w, h) of the resizes ``utils.utils.img_resize`` applies to an image of ``size_wh``, in order, with
    its own int() / floor arithmetic: the shrink to ``max_size`` (if the long edge is larger), then the floor to a multiple
    of ``down_scale``."""
    w, h = int(size_wh[0]), int(size_wh[1])
    steps = []
    if max(w, h) > max_size:
        w0, h0 = w, h
        w = int(1.0 * w0 / max(w0, h0) * max_size)
        h = int(1.0 * h0 / max(w0, h0) * max_size)
        steps.append((w, h))
    if down_scale is not None:
        w = w // down_scale * down_scale
        h = h // down_scale * down_scale
        steps.append((w, h))
    return steps


def img_resize_size(size_wh, max_size, down_scale=None):
    """``img_resize(img, max_size, down_scale).size`` for an image of ``size_wh``."""
    steps = img_resize_steps(size_wh, max_size, down_scale)
    return steps[-1] if steps else (int(size_wh[0]), int(size_wh[1]))


def device_supported(size_wh, max_size, down_scale=None):
    """Whether every step of the resize is inside the kernels' limits (positive sizes, a shrink of at most 16 per axis)."""
    w, h = int(size_wh[0]), int(size_wh[1])
    for tw, th in img_resize_steps(size_wh, max_size, down_scale):
        if tw <= 0 or th <= 0 or w > MAX_SHRINK * tw or h > MAX_SHRINK * th:
            return False
        w, h = tw, th
    return w > 0 and h > 0


# ------------------------------------------------------------------------------------------------ coefficient tables
_host_tables = {}            # (kind, in, out) -> (ksize, bounds int32 [out,2], coefficients [out,ksize])
_dev_tables = {}             # (kind, device, (in, out) pairs) -> int32 device tensor: the pairs' tables one after the other


def coeffs_u8(in_size, out_size):
    """Pillow's 8-bit bicubic table for one axis: (ksize, bounds int32 [out,2] = (first, count), kk int32 [out,ksize])."""
    return _coeffs("u8", in_size, out_size)


def coeffs_u8_bilinear(in_size, out_size):
    """Pillow's 8-bit bilinear (triangle) table for one axis, laid out like coeffs_u8's."""
    return _coeffs("u8_bilinear", in_size, out_size)


def coeffs_f32(in_size, out_size):
    """The antialiased bicubic weights of F.interpolate for one axis: (ksize, bounds int32 [out,2], w float32 [out,ksize])."""
    return _coeffs("f32", in_size, out_size)


def coeffs_f64(in_size, out_size):
    """Pillow's normalised double weights for one axis, the numbers coeffs_u8 rounds to 22 bits: (ksize, bounds int32 [out,2], w
    float64 [out,ksize]).  The deep resize's table (img_resize_float, yuv.DeepImgResize)."""
    return _coeffs("f64", in_size, out_size)


def _coeffs(kind, in_size, out_size):
    key = (kind, int(in_size), int(out_size))
    t = _host_tables.get(key)
    if t is None:
        fn = getattr(_lib.lib(), "vst_resize_coeffs_" + kind)
        ks = C.c_int(0)
        _lib.check(fn(key[1], key[2], C.byref(ks), None, None), f"vst_resize_coeffs_{kind}")
        bounds = np.empty((key[2], 2), np.int32)
        co = np.empty((key[2], ks.value), {"f32": np.float32, "f64": np.float64}.get(kind, np.int32))
        _lib.check(fn(key[1], key[2], C.byref(ks), C.c_void_p(bounds.ctypes.data), C.c_void_p(co.ctypes.data)),
                   f"vst_resize_coeffs_{kind}")
        t = _host_tables[key] = (ks.value, bounds, co)
    return t


def _tables_on(kind, device, pairs):
    """The tables of the (in, out) pairs, concatenated in the order the entry points read them, on `device` (uploaded once)."""
    import torch
    key = (kind, str(device), tuple(pairs))
    t = _dev_tables.get(key)
    if t is None:
        words = []
        for a, b in pairs:
            _, bounds, co = _coeffs(kind, a, b)
            words += [bounds.reshape(-1), co.reshape(-1).view(np.int32)]
        host = np.concatenate(words) if words else np.zeros(1, np.int32)
        t = _dev_tables[key] = torch.from_numpy(host).to(device)
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(stream):
    import torch
    if stream is None:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))


def _check_u8_frame(src):
    import torch
    if not torch.is_tensor(src) or not src.is_cuda or src.dtype != torch.uint8:
        raise ValueError("src must be a uint8 tensor on the GPU (no CPU fallback)")
    if src.dim() == 4 and src.shape[0] == 1:
        src = src[0]
    if src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise ValueError(f"expected a contiguous [H,W,3] frame, got {tuple(src.shape)}")
    return src


# ------------------------------------------------------------------------------------------------ input side: PIL, bit-exact
def resize_u8(src_dev_u8, size_wh, stream=None, out=None, tmp=None):
    """``Image.resize(size_wh, Image.BICUBIC)`` of a uint8 [H,W,3] device frame, byte for byte.  `out` (uint8 [h,w,3]) and
    `tmp` (uint8, at least H*w*3 bytes) are allocated when not given."""
    import torch
    src = _check_u8_frame(src_dev_u8)
    Hs, Ws = int(src.shape[0]), int(src.shape[1])
    Wd, Hd = int(size_wh[0]), int(size_wh[1])
    if out is None:
        out = torch.empty((Hd, Wd, 3), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.numel() != Hd * Wd * 3 or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"out must be a contiguous uint8 tensor of {Hd}x{Wd}x3 on {src.device}")
    pairs = [p for p in ((Ws, Wd), (Hs, Hd)) if p[0] != p[1]]
    with torch.cuda.device(src.device):
        tables = _tables_on("u8", src.device, pairs) if pairs else None
        if len(pairs) == 2 and tmp is None:
            tmp = torch.empty(Hs * Wd * 3, dtype=torch.uint8, device=src.device)
        if tmp is not None and len(pairs) == 2 and (tmp.dtype != torch.uint8 or tmp.numel() < Hs * Wd * 3):
            raise ValueError("tmp is too small")
        _lib.check(_lib.lib().vst_resize_u8(_ptr(src), Hs, Ws, _ptr(out), Hd, Wd, _ptr(tables), _ptr(tmp), _stream(stream)),
                   "vst_resize_u8")
    return out


def resize_grey_u8(src_dev_u8, size_wh, stream=None, out=None, tmp=None):
    """``Image.resize(size_wh, Image.BILINEAR)`` of an "L" image, a uint8 [H,W] device tensor, byte for byte (a frame's matte on
    its way to the stylised size).  `out` (uint8 [h,w]) and `tmp` (uint8, at least H*w bytes) are allocated when not given."""
    import torch
    src = src_dev_u8
    if not torch.is_tensor(src) or not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 2 or not src.is_contiguous():
        raise ValueError("src must be a contiguous uint8 [H,W] tensor on the GPU (no CPU fallback)")
    Hs, Ws = int(src.shape[0]), int(src.shape[1])
    Wd, Hd = int(size_wh[0]), int(size_wh[1])
    if out is None:
        out = torch.empty((Hd, Wd), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.numel() != Hd * Wd or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"out must be a contiguous uint8 tensor of {Hd}x{Wd} on {src.device}")
    pairs = [p for p in ((Ws, Wd), (Hs, Hd)) if p[0] != p[1]]
    with torch.cuda.device(src.device):
        tables = _tables_on("u8_bilinear", src.device, pairs) if pairs else None
        if len(pairs) == 2 and tmp is None:
            tmp = torch.empty(Hs * Wd, dtype=torch.uint8, device=src.device)
        if tmp is not None and len(pairs) == 2 and (tmp.dtype != torch.uint8 or tmp.numel() < Hs * Wd):
            raise ValueError("tmp is too small")
        _lib.check(_lib.lib().vst_resize_grey_u8(_ptr(src), Hs, Ws, _ptr(out), Hd, Wd, _ptr(tables), _ptr(tmp), _stream(stream)),
                   "vst_resize_grey_u8")
    return out


def grey_device_supported(src_hw, dst_hw):
    """Whether resize_grey_u8 takes a map of src_hw to dst_hw (a shrink of at most MAX_SHRINK per axis)."""
    return all(0 < d and 0 < s <= MAX_SHRINK * d for s, d in zip(src_hw, dst_hw))


class DeviceImgResize:
    """``img_resize`` for frames of ONE source size with every buffer made up front: the intermediate of the two steps and
    the pass buffer belong to this object, so one object serves one frame at a time (a pipeline keeps one per ring slot)."""

    def __init__(self, src_hw, max_size, down_scale, device):
        import torch
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.steps = img_resize_steps((self.src_hw[1], self.src_hw[0]), max_size, down_scale)
        self.size_wh = self.steps[-1] if self.steps else (self.src_hw[1], self.src_hw[0])
        if not device_supported((self.src_hw[1], self.src_hw[0]), max_size, down_scale):
            raise _lib.VstError(f"a {self.src_hw[1]}x{self.src_hw[0]} frame to max_size {max_size} is outside the device "
                                f"resize's limits (shrink factor above {MAX_SHRINK})")
        h, tmp_bytes = self.src_hw[0], 1
        for tw, th in self.steps:
            tmp_bytes = max(tmp_bytes, h * tw * 3)
            h = th
        with torch.cuda.device(device):
            self.tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=device)
            self.mid = [torch.empty((th, tw, 3), dtype=torch.uint8, device=device) for tw, th in self.steps[:-1]]

    def __call__(self, src, out, stream=None):
        """src uint8 [H,W,3] -> out uint8 [h,w,3] (or [1,h,w,3]), queued on the current stream."""
        src = _check_u8_frame(src)
        if tuple(src.shape[:2]) != self.src_hw:
            raise ValueError(f"made for {self.src_hw} frames, got {tuple(src.shape[:2])}")
        if not self.steps:
            out.view(src.shape).copy_(src, non_blocking=True)
            return out
        cur = src
        for n, wh in enumerate(self.steps):
            dst = out if n == len(self.steps) - 1 else self.mid[n]
            resize_u8(cur, wh, stream=stream, out=dst, tmp=self.tmp)
            cur = dst
        return out


def img_resize_device(src_dev_u8, max_size, down_scale=None, stream=None):
    """``utils.utils.img_resize`` of a uint8 [H,W,3] device frame: the same two-step rule and sizes, the same bytes."""
    src = _check_u8_frame(src_dev_u8)
    cur = src
    for wh in img_resize_steps((src.shape[1], src.shape[0]), max_size, down_scale):
        cur = resize_u8(cur, wh, stream=stream)
    return cur.clone() if cur is src else cur


# ------------------------------------------------------------------------------------------------ input side: float (deep frames)
def float_passes(size_wh, max_size, down_scale=None):
    """The passes of ``img_resize`` in float on an image of ``size_wh``, in order: (axis, in, out) with axis 1 = horizontal, 0 =
    vertical.  Every step of img_resize_steps whose size differs from its input is a horizontal pass, then a vertical one; an
    axis that does not change has no pass.  Raises VstError for a step outside the limits (sizes only shrink, by at most 16)."""
    w, h = int(size_wh[0]), int(size_wh[1])
    if not device_supported((w, h), max_size, down_scale):
        raise _lib.VstError(f"a {w}x{h} frame to max_size {max_size} is outside the float resize's limits: a step may shrink an "
                            f"axis by a factor of {MAX_SHRINK} at the most (VST_RESIZE_MAX_SHRINK)")
    passes = []
    for tw, th in img_resize_steps((w, h), max_size, down_scale):
        if tw != w:
            passes.append((1, w, tw))
        if th != h:
            passes.append((0, h, th))
        w, h = tw, th
    return passes


def img_resize_float(rgb, max_size, down_scale=None):
    """``utils.utils.img_resize`` restated in float64 on an [H,W,3] (or [H,W]) array, the arithmetic of vst_yuv16_img_resize_f32
    (vstnet.h, "Deep resize") without its roundings to fp32: the size rule of img_resize_steps, every pass with Pillow's
    normalised double weights (coeffs_f64), nothing clamped or quantised anywhere - the passes are linear, so the scale of the
    input (0..1, 0..255) is the caller's, and so is the final clamp.  The tests' reference, and what ``video_transfer.py
    --stub_stylise`` rehearses the deep resize with."""
    x = np.asarray(rgb, np.float64)
    if x.ndim not in (2, 3):
        raise ValueError(f"expected an [H, W, 3] frame, got {tuple(x.shape)}")
    for axis, n_in, n_out in float_passes((x.shape[1], x.shape[0]), max_size, down_scale):
        _, bounds, w = coeffs_f64(n_in, n_out)
        m = np.zeros((n_out, n_in), np.float64)         # the pass as a matrix: row i holds its taps at first_i .. first_i + n_i
        for i, (first, n) in enumerate(bounds):
            m[i, first:first + n] = w[i, :n]
        x = np.moveaxis(np.tensordot(m, x, axes=(1, axis)), 0, axis)
    return x


# ------------------------------------------------------------------------------------------------ output side: float -> writer
def resize_float(x_hwc, size_hw):
    """``resize_f32`` stated in numpy on an [H,W,3] array: the same fp32 weights (coeffs_f32), float64 accumulation, horizontal
    pass first, an axis of equal size left alone.  What ``video_transfer.py --stub_stylise`` rehearses the resize to the written
    size of a deep frame with."""
    x = np.asarray(x_hwc, np.float64)
    for axis, n_out in ((1, int(size_hw[1])), (0, int(size_hw[0]))):
        n_in = x.shape[axis]
        if n_in == n_out:
            continue
        _, bounds, w = coeffs_f32(n_in, n_out)
        m = np.zeros((n_out, n_in), np.float64)
        for i, (first, n) in enumerate(bounds):
            m[i, first:first + n] = w[i, :n]
        x = np.moveaxis(np.tensordot(m, x, axes=(1, axis)), 0, axis)
    return x


def _resize_f32(x, size_hw, to_u8, stream, out, tmp):
    import torch
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("x must be a float32 [B,3,H,W] tensor on the GPU (no CPU fallback)")
    x = x.contiguous()
    B, _, Hs, Ws = (int(v) for v in x.shape)
    Hd, Wd = int(size_hw[0]), int(size_hw[1])
    shape = (B, Hd, Wd, 3) if to_u8 else (B, 3, Hd, Wd)
    dtype = torch.uint8 if to_u8 else torch.float32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=x.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape}")
    pairs = ([(Ws, Wd)] if Ws != Wd else []) + [(Hs, Hd)]
    with torch.cuda.device(x.device):
        tables = _tables_on("f32", x.device, pairs)
        if Ws != Wd and tmp is None:
            tmp = torch.empty(B * 3 * Hs * Wd, dtype=torch.float32, device=x.device)
        if Ws != Wd and (tmp.dtype != torch.float32 or tmp.numel() < B * 3 * Hs * Wd):
            raise ValueError("tmp is too small")
        fn = _lib.lib().vst_resize_f32_to_u8 if to_u8 else _lib.lib().vst_resize_f32
        _lib.check(fn(_ptr(x), B, Hs, Ws, _ptr(out), Hd, Wd, _ptr(tables), _ptr(tmp), _stream(stream)),
                   "vst_resize_f32_to_u8" if to_u8 else "vst_resize_f32")
    return out


def resize_to_u8(x_planar, size_hw, stream=None, out=None, tmp=None):
    """float32 [B,3,H,W] -> uint8 [B,h,w,3]: antialiased bicubic (align_corners=False) with fp32 accumulation, then * 255,
    clamp to [0, 255], truncate - what ``F.interpolate(..., antialias=True).mul(255).clamp(0, 255).byte()`` and the HWC
    permute compute, with double-built weights."""
    return _resize_f32(x_planar, size_hw, True, stream, out, tmp)


def resize_f32(x_planar, size_hw, stream=None, out=None, tmp=None):
    """The same resize without the quantising epilogue: float32 [B,3,h,w]."""
    return _resize_f32(x_planar, size_hw, False, stream, out, tmp)
