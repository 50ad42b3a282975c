"""Guided upscale on the device (csrc/guided.hip; DESIGN.md section 6, "Guided upscale"): a stylisation made at a working size
carried over to the source frame's size by He and Sun's fast guided filter with a colour guide.

``guided_fit`` fits, per working-size pixel, the 3x3 matrix and offset that map the working-size content (the guide) to the
working-size stylised frame, and smooths them; ``guided_apply`` samples those 12 planes bilinearly at the full size and applies
them to the source frame, so the stylisation carries over while edges and texture come from the source.  ``GuidedUpscale`` owns
the buffers of one frame in flight.  Every call is queued on the current stream (or the one given) and never synchronises.
There is no CPU fallback: tensors off the GPU raise ``ValueError``, a shape the kernels do not take raises ``VstError``.

The defaults (radius 4, eps 1e-3) are starting values: picture quality has not been measured.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .resize import _check_u8_frame, _ptr, _stream

MAX_RADIUS = _lib.GUIDED_MAX_RADIUS
DEFAULT_RADIUS = 4
DEFAULT_EPS = 1e-3


def workspace_bytes(h, w, radius):
    """The bytes of device memory a fit of an h x w frame needs (vst_guided_workspace_bytes; needs no GPU)."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().vst_guided_workspace_bytes(int(h), int(w), int(radius), C.byref(n)), "vst_guided_workspace_bytes")
    return int(n.value)


def _check_target(target, h, w):
    import torch
    if not torch.is_tensor(target) or not target.is_cuda or target.dtype != torch.float32:
        raise ValueError("target must be a float32 tensor on the GPU (no CPU fallback)")
    if target.dim() == 4 and target.shape[0] == 1:
        target = target[0]
    if tuple(target.shape) != (3, h, w) or not target.is_contiguous():
        raise ValueError(f"expected a contiguous [3,{h},{w}] target, got {tuple(target.shape)}")
    return target


def guided_fit(guide_u8, target_f32, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, out=None, ws=None, stream=None):
    """The coefficient planes float32 [12,h,w] that map guide_u8 (uint8 [h,w,3] or [1,h,w,3]) to target_f32 (float32 [3,h,w] or
    [1,3,h,w]): planes 3 k + c hold A[k][c], planes 9 + c hold b[c] (vstnet.h, "Guided upscale").  `out` and `ws` (uint8, at
    least workspace_bytes(h, w, radius) bytes) are allocated when not given."""
    import torch
    guide = _check_u8_frame(guide_u8)
    h, w = int(guide.shape[0]), int(guide.shape[1])
    target = _check_target(target_f32, h, w)
    if target.device != guide.device:
        raise ValueError("guide and target are on different devices")
    need = workspace_bytes(h, w, radius)
    if out is None:
        out = torch.empty((12, h, w), dtype=torch.float32, device=guide.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (12, h, w) or not out.is_contiguous() or out.device != guide.device:
        raise ValueError(f"out must be a contiguous float32 [12,{h},{w}] tensor on {guide.device}")
    with torch.cuda.device(guide.device):
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=guide.device)
        elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.device != guide.device:
            raise ValueError(f"ws must be a contiguous uint8 tensor of at least {need} bytes on {guide.device}")
        _lib.check(_lib.lib().vst_guided_fit(_ptr(guide), _ptr(target), h, w, int(radius), float(eps), _ptr(out), _ptr(ws),
                                             _stream(stream)), "vst_guided_fit")
    return out


def guided_apply(coef, src_u8, out=None, to_u8=True, stream=None):
    """coef (float32 [12,h,w]) applied to src_u8 (uint8 [H,W,3] or [1,H,W,3], H >= h, W >= w): uint8 [1,H,W,3] under the writer's
    epilogue (* 255, clamp, truncate), or with to_u8=False float32 [1,3,H,W]."""
    import torch
    src = _check_u8_frame(src_u8)
    H, W = int(src.shape[0]), int(src.shape[1])
    if not torch.is_tensor(coef) or not coef.is_cuda or coef.dtype != torch.float32 or coef.dim() != 3 or coef.shape[0] != 12 \
            or not coef.is_contiguous() or coef.device != src.device:
        raise ValueError(f"coef must be a contiguous float32 [12,h,w] tensor on {src.device} (guided_fit)")
    h, w = int(coef.shape[1]), int(coef.shape[2])
    shape = (1, H, W, 3) if to_u8 else (1, 3, H, W)
    dtype = torch.uint8 if to_u8 else torch.float32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=src.device)
    elif out.dtype != dtype or out.numel() != 3 * H * W or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on {src.device}")
    name = "vst_guided_apply_u8" if to_u8 else "vst_guided_apply_f32"
    with torch.cuda.device(src.device):
        _lib.check(getattr(_lib.lib(), name)(_ptr(coef), h, w, _ptr(src), H, W, _ptr(out), _stream(stream)), name)
    return out.view(shape)


class GuidedUpscale:
    """The guided upscale of frames of ONE working size to ONE source size with every buffer made up front: the coefficient
    planes and the fit's workspace belong to this object, so one object serves one frame at a time (a pipeline keeps one per
    ring slot, like resize.DeviceImgResize)."""

    def __init__(self, work_hw, src_hw, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=None):
        import torch
        self.work_hw = (int(work_hw[0]), int(work_hw[1]))
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.radius, self.eps = int(radius), float(eps)
        if self.radius != radius or not 1 <= self.radius <= MAX_RADIUS:
            raise ValueError(f"radius must be an integer in 1..{MAX_RADIUS}, got {radius}")
        if not 0.0 < self.eps < float("inf"):
            raise ValueError(f"eps must be positive and finite, got {eps}")
        if self.src_hw[0] < self.work_hw[0] or self.src_hw[1] < self.work_hw[1]:
            raise ValueError(f"the source size {self.src_hw} is smaller than the working size {self.work_hw}: nothing to upscale")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        need = workspace_bytes(self.work_hw[0], self.work_hw[1], self.radius)
        with torch.cuda.device(self.device):
            self.coef = torch.empty((12,) + self.work_hw, dtype=torch.float32, device=self.device)
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)

    def __call__(self, content_u8, stylised_f32, src_u8, out=None, stream=None):
        """content_u8 uint8 [h,w,3], stylised_f32 float32 [3,h,w] (either with a leading 1), src_u8 uint8 [H,W,3] -> uint8
        [1,H,W,3], queued on the current stream."""
        src = _check_u8_frame(src_u8)
        if tuple(src.shape[:2]) != self.src_hw:
            raise ValueError(f"made for {self.src_hw} source frames, got {tuple(src.shape[:2])}")
        guide = _check_u8_frame(content_u8)
        if tuple(guide.shape[:2]) != self.work_hw:
            raise ValueError(f"made for {self.work_hw} working frames, got {tuple(guide.shape[:2])}")
        guided_fit(guide, stylised_f32, self.radius, self.eps, out=self.coef, ws=self.ws, stream=stream)
        return guided_apply(self.coef, src, out=out, to_u8=True, stream=stream)
