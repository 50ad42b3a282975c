"""Optical flow on the device (csrc/flow.hip; DESIGN.md section 6, "Optical flow"): a dense coarse-to-fine, warping Lucas-Kanade
estimator on a pair of uint8 frames and the forward-backward consistency mask, so that the temporal loss (vstnet_amd.temporal)
can be pointed at footage that comes without flow files.

Frames are uint8 [h,w,3]; a flow is float32 [2,h,w] with the x displacement first, in the convention of ``temporal.warp`` and
``temporal.temporal_loss``: ``ref(p) ~ src(p - flow(p))``, so ``estimate_flow(frame t, frame t-1)`` is the flow that
``temporal_loss(frame t-1, frame t, flow)`` expects.  A mask is uint8 [h,w], 1 where the forward and the backward flow agree.
Every call is queued on the current stream and never waits for the card.  There is no CPU fallback: tensors off the GPU raise
``ValueError``, parameters the kernels do not take raise ``VstError``.

The defaults (5 levels, 3 iterations, radius 3, lambda 1e-3) are starting values checked on synthetic textures under smooth
motion only; see DESIGN.md for what is measured and what is not."""
from __future__ import annotations

import ctypes as C

from . import _lib
from .resize import _ptr, _stream
from .temporal import _check_like, _device

DEFAULTS = {"levels": 5, "iters": 3, "radius": 3, "lam": 1e-3}


def workspace_bytes(h, w, levels=DEFAULTS["levels"]):
    """The bytes of device memory an estimate_flow call on an h x w pair needs (vst_flow_workspace_bytes; needs no GPU)."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().vst_flow_workspace_bytes(int(h), int(w), int(levels), C.byref(n)), "vst_flow_workspace_bytes")
    return int(n.value)


def level_count(h, w, levels=DEFAULTS["levels"]):
    """The levels the pyramid of an h x w frame really has: one is added while fewer than `levels` exist and the new level's
    shorter edge is at least 8."""
    n = 1
    while n < int(levels):
        h, w = (int(h) + 1) // 2, (int(w) + 1) // 2
        if min(h, w) < 8:
            break
        n += 1
    return n


def _check_u8(x, what):
    import torch
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.uint8:
        raise ValueError(f"{what} must be a uint8 [h,w,3] tensor on the GPU (no CPU fallback)")
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 3 or x.shape[2] != 3 or not x.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous uint8 [h,w,3] frame, got {tuple(x.shape)}")
    return x


def _check_ws(ws, need, dev):
    import torch
    if ws is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if not torch.is_tensor(ws) or ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.device != dev:
        raise ValueError(f"ws must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    return ws


def estimate_flow(ref_u8, src_u8, levels=DEFAULTS["levels"], iters=DEFAULTS["iters"], radius=DEFAULTS["radius"],
                  lam=DEFAULTS["lam"], out=None, ws=None):
    """The flow of the pair (ref = frame t, src = frame t-1), float32 [2,h,w]: ref(p) ~ src(p - flow(p)).  `out` and `ws` (uint8,
    at least workspace_bytes(h, w, levels) bytes) are allocated when not given."""
    import torch
    ref = _check_u8(ref_u8, "ref_u8")
    src = _check_like(_check_u8(src_u8, "src_u8"), ref, "src_u8")
    h, w = int(ref.shape[0]), int(ref.shape[1])
    dev = ref.device
    need = workspace_bytes(h, w, levels)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((2, h, w), dtype=torch.float32, device=dev)
        out = _check_like(out, ref, "out", (2, h, w), torch.float32)
        ws = _check_ws(ws, need, dev)
        _lib.check(_lib.lib().vst_flow_lk_u8(_ptr(ref), _ptr(src), h, w, int(levels), int(iters), int(radius), float(lam),
                                             _ptr(out), _ptr(ws), _stream(None)), "vst_flow_lk_u8")
    return out


def consistency(flow_fwd, flow_bwd, out=None):
    """The forward-backward mask, uint8 [h,w]: flow_fwd = estimate_flow(t, t-1), flow_bwd = estimate_flow(t-1, t); 1 where p -
    fwd(p) lies inside the frame and |fwd + bwd(p - fwd)|^2 <= 0.01 (|fwd|^2 + |bwd(p - fwd)|^2) + 0.5."""
    import torch
    if not torch.is_tensor(flow_fwd) or not flow_fwd.is_cuda or flow_fwd.dtype != torch.float32 or flow_fwd.dim() != 3 \
            or flow_fwd.shape[0] != 2 or not flow_fwd.is_contiguous():
        raise ValueError("flow_fwd must be a contiguous float32 [2,h,w] tensor on the GPU (no CPU fallback)")
    h, w = int(flow_fwd.shape[1]), int(flow_fwd.shape[2])
    bwd = _check_like(flow_bwd, flow_fwd, "flow_bwd")
    dev = flow_fwd.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((h, w), dtype=torch.uint8, device=dev)
        out = _check_like(out, flow_fwd, "out", (h, w), torch.uint8)
        _lib.check(_lib.lib().vst_flow_consistency(_ptr(flow_fwd), _ptr(bwd), h, w, _ptr(out), _stream(None)),
                   "vst_flow_consistency")
    return out


class FlowEstimator:
    """The estimator for pairs of ONE size with its workspace, its flow and (mask=True) its backward flow and mask made up
    front, so one object serves one pair at a time (a pipeline keeps one per ring slot, like temporal.TemporalLoss).  Calls
    with an `out` of their own may follow one another on one stream."""

    def __init__(self, hw, levels=DEFAULTS["levels"], iters=DEFAULTS["iters"], radius=DEFAULTS["radius"], lam=DEFAULTS["lam"],
                 mask=False, device=None):
        import torch
        self.hw = (int(hw[0]), int(hw[1]))
        self.params = {"levels": int(levels), "iters": int(iters), "radius": int(radius), "lam": float(lam)}
        self.device = _device(device)
        if self.device.type != "cuda":
            raise ValueError("the flow is estimated on the GPU (no CPU fallback)")
        need = workspace_bytes(self.hw[0], self.hw[1], levels)
        with torch.cuda.device(self.device):
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.flow = torch.empty((2,) + self.hw, dtype=torch.float32, device=self.device)
            self.backward = self.valid = None
            if mask:
                self.backward = torch.empty((2,) + self.hw, dtype=torch.float32, device=self.device)
                self.valid = torch.empty(self.hw, dtype=torch.uint8, device=self.device)

    def __call__(self, ref_u8, src_u8, out=None):
        """-> the flow of (ref, src) (this object's, or `out`); queued on the current stream."""
        if tuple(ref_u8.shape[-3:-1]) != self.hw:
            raise ValueError(f"made for {self.hw} frames, got {tuple(ref_u8.shape[-3:-1])}")
        return estimate_flow(ref_u8, src_u8, out=self.flow if out is None else out, ws=self.ws, **self.params)

    def masked(self, ref_u8, src_u8, out=None):
        """-> (flow, valid): the flow of (ref, src), the flow of the swapped pair into this object's buffer, and their mask."""
        if self.valid is None:
            raise ValueError("made without mask=True")
        flow = self(ref_u8, src_u8, out=out)
        self(src_u8, ref_u8, out=self.backward)     # (the workspace is free again: one stream, one call after the other)
        return flow, consistency(flow, self.backward, out=self.valid)
