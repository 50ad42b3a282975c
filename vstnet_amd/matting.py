"""Matting-Laplacian affinity loss on the device (csrc/matting.hip; DESIGN.md section 6, "Affinity loss"): the reference's measure
of photorealism, ``sum_c x_c^T L x_c / (H W)`` with L Levin's Matting Laplacian of the content image, and its gradient
``2 L x / (H W)`` - how far a stylised image x is from being a locally affine function of the content in every window.

``matting_loss`` takes the content as a uint8 frame and x either as the float32 planar stylised frame or as a written uint8
frame, and returns the three per-channel values (their sum is the reference's loss) as a device fp64 tensor.  ``MattingLoss``
owns the buffers of one frame in flight.  Every call is queued on the current stream (or the one given) and never synchronises.
There is no CPU fallback: tensors off the GPU raise ``ValueError``, a shape the kernels do not take raises ``VstError``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .resize import _check_u8_frame, _ptr, _stream

MAX_RADIUS = _lib.MATTING_MAX_RADIUS
DEFAULT_RADIUS = 1              # the reference's win_rad
DEFAULT_EPS = 1e-7              # the reference's eps


def workspace_bytes(h, w, radius):
    """The bytes of device memory a call on an h x w frame needs (vst_matting_workspace_bytes; needs no GPU)."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().vst_matting_workspace_bytes(int(h), int(w), int(radius), C.byref(n)), "vst_matting_workspace_bytes")
    return int(n.value)


def _check_params(radius, eps):
    if int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"radius must be an integer in 1..{MAX_RADIUS}, got {radius}")
    if not 0.0 < float(eps) < float("inf"):
        raise ValueError(f"eps must be positive and finite, got {eps}")
    return int(radius), float(eps)


def _check_x(x, h, w):
    """x as the kernels read it: (tensor, True) for a uint8 [h,w,3] frame, (tensor, False) for a float32 [3,h,w] one"""
    import torch
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype not in (torch.float32, torch.uint8):
        raise ValueError("x must be a float32 [3,h,w] or uint8 [h,w,3] tensor on the GPU (no CPU fallback)")
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    want = (h, w, 3) if x.dtype == torch.uint8 else (3, h, w)
    if tuple(x.shape) != want or not x.is_contiguous():
        raise ValueError(f"expected a contiguous {x.dtype} tensor of shape {want}, got {tuple(x.shape)}")
    return x, x.dtype == torch.uint8


def matting_loss(guide_u8, x, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, grad=False, out=None, grad_out=None, ws=None, stream=None):
    """x_c^T L x_c / (h w) per channel, a device float64 [3] tensor, with L the Matting Laplacian of guide_u8 (uint8 [h,w,3] or
    [1,h,w,3]); x is float32 [3,h,w] / [1,3,h,w] or uint8 [h,w,3] / [1,h,w,3] (read as v / 255).  With grad=True returns
    (loss3, gradient) with the gradient 2 L x / (h w) as float32 [3,h,w].  `out`, `grad_out` and `ws` (uint8, at least
    workspace_bytes(h, w, radius) bytes) are allocated when not given."""
    import torch
    guide = _check_u8_frame(guide_u8)
    h, w = int(guide.shape[0]), int(guide.shape[1])
    x, is_u8 = _check_x(x, h, w)
    dev = guide.device
    if x.device != dev:
        raise ValueError("guide and x are on different devices")
    need = workspace_bytes(h, w, radius)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(3, dtype=torch.float64, device=dev)
        elif out.dtype != torch.float64 or out.numel() != 3 or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous float64 [3] tensor on {dev}")
        if not grad:
            if grad_out is not None:
                raise ValueError("grad_out given without grad=True")
        elif grad_out is None:
            grad_out = torch.empty((3, h, w), dtype=torch.float32, device=dev)
        elif grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (3, h, w) or not grad_out.is_contiguous() \
                or grad_out.device != dev:
            raise ValueError(f"grad_out must be a contiguous float32 [3,{h},{w}] tensor on {dev}")
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.device != dev:
            raise ValueError(f"ws must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
        name = "vst_matting_loss_u8" if is_u8 else "vst_matting_loss_f32"
        _lib.check(getattr(_lib.lib(), name)(_ptr(guide), _ptr(x), h, w, int(radius), float(eps), _ptr(out), _ptr(grad_out),
                                             _ptr(ws), _stream(stream)), name)
    return (out, grad_out) if grad else out


class MattingLoss:
    """The affinity loss of frames of ONE size with every buffer made up front: the three values, the gradient (grad=True) and
    the workspace belong to this object, so one object serves one frame at a time (a pipeline keeps one per ring slot, like
    guided.GuidedUpscale)."""

    def __init__(self, hw, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=None, grad=False):
        import torch
        self.hw = (int(hw[0]), int(hw[1]))
        self.radius, self.eps = _check_params(radius, eps)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        need = workspace_bytes(self.hw[0], self.hw[1], self.radius)
        with torch.cuda.device(self.device):
            self.loss = torch.empty(3, dtype=torch.float64, device=self.device)
            self.grad = torch.empty((3,) + self.hw, dtype=torch.float32, device=self.device) if grad else None
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)

    def __call__(self, guide_u8, x, out=None, stream=None):
        """-> the float64 [3] tensor (this object's, or `out`), or with grad=True the pair; queued on the current stream."""
        guide = _check_u8_frame(guide_u8)
        if tuple(guide.shape[:2]) != self.hw:
            raise ValueError(f"made for {self.hw} frames, got {tuple(guide.shape[:2])}")
        return matting_loss(guide, x, self.radius, self.eps, grad=self.grad is not None, out=self.loss if out is None else out,
                            grad_out=self.grad, ws=self.ws, stream=stream)
