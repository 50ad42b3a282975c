"""Temporal loss on the device (csrc/temporal.hip; DESIGN.md section 6, "Temporal loss"): the reference's measure of flicker under
known motion (utils/TemporalLoss.py) - ``mean |warp(first, flow) - second|``, its ``warp`` (nearest sampling with border padding
and the reference's W - 1 / align_corners=False quirk), the smooth random flow of ``GenerateFakeFlow`` and a short synthetic clip
made by chaining ``GenerateFakeData``.

Frames are uint8 [h,w,3] or float32 [3,h,w]; a flow is float32 [2,h,w] with the x displacement first: pixel x of the warped frame
is the frame sampled at ``x - flow(x)``.  ``temporal_loss`` returns the three per-channel means as a device float64 tensor (the
reference's scalar is their mean, ``mean3``).  ``TemporalLoss`` owns the buffers of one frame in flight.  Every call is queued on
the current stream - ``torch.cuda.stream`` is the one way to pick another, so what a call allocates belongs to the stream its
kernels run on - and never waits for the card.  Two uploads block the host for the length of a small copy from pageable memory,
not for queued work: the coarse grid of ``fake_flow_from`` (a few hundred bytes) and the still of ``synthetic_clip``.  There is
no CPU fallback: tensors off the GPU raise ``ValueError``, a shape the kernels do not take raises ``VstError``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .resize import _ptr, _stream


def workspace_bytes(h, w):
    """The bytes of device memory a temporal_loss call on an h x w frame needs (vst_temporal_workspace_bytes; needs no GPU)."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().vst_temporal_workspace_bytes(int(h), int(w), C.byref(n)), "vst_temporal_workspace_bytes")
    return int(n.value)


def fake_flow_workspace_bytes(h, w, gh, gw, ksize):
    """The bytes of device memory a fake_flow call needs (vst_fake_flow_workspace_bytes; needs no GPU)."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().vst_fake_flow_workspace_bytes(int(h), int(w), int(gh), int(gw), int(ksize), C.byref(n)),
               "vst_fake_flow_workspace_bytes")
    return int(n.value)


def _device(device):
    """the device with its index filled in: tensors report cuda:0 where a caller said cuda"""
    import torch
    d = torch.device(device if device is not None else "cuda")
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def mean3(loss3):
    """The reference's scalar from the three per-channel means: (r + g + b) / 3 in fp64, in that order."""
    v = [float(x) for x in loss3]
    return (v[0] + v[1] + v[2]) / 3.0


def _check_frame(x, what="x"):
    """x as the kernels read it: (tensor, is_u8, h, w) for a uint8 [h,w,3] or a float32 [3,h,w] frame"""
    import torch
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{what} must be a float32 [3,h,w] or uint8 [h,w,3] tensor on the GPU (no CPU fallback)")
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    is_u8 = x.dtype == torch.uint8
    if x.dim() != 3 or x.shape[2 if is_u8 else 0] != 3 or not x.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous uint8 [h,w,3] or float32 [3,h,w] frame, got {x.dtype} {tuple(x.shape)}")
    h, w = (int(x.shape[0]), int(x.shape[1])) if is_u8 else (int(x.shape[1]), int(x.shape[2]))
    return x, is_u8, h, w


def _check_like(t, like, what, shape=None, dtype=None):
    import torch
    shape = tuple(like.shape) if shape is None else shape
    dtype = like.dtype if dtype is None else dtype
    if t is None:
        return None
    if not torch.is_tensor(t) or t.device != like.device or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} tensor on {like.device}")
    if t.dim() == len(shape) + 1 and t.shape[0] == 1:
        t = t[0]
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    return t


def warp(x, flow, noise=None, out=None):
    """The reference's warp(x, flo) of one frame - grid_sample(mode='nearest', padding_mode='border') on its grid - with `noise`
    (float32 [3,h,w], in units of the 0..1 range) added after it: v + noise for a float frame, clamp(rint(v + 255 noise), 0, 255)
    for a uint8 one.  flow None: no warp.  Returns `out` (allocated when not given; never x itself)."""
    import torch
    x, is_u8, h, w = _check_frame(x)
    flow = _check_like(flow, x, "flow", (2, h, w), torch.float32)
    noise = _check_like(noise, x, "noise", (3, h, w), torch.float32)
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty_like(x)
        out = _check_like(out, x, "out")
        if out.data_ptr() == x.data_ptr():
            raise ValueError("out must not be x: the warp gathers")
        name = "vst_warp_u8" if is_u8 else "vst_warp_f32"
        _lib.check(getattr(_lib.lib(), name)(_ptr(x), _ptr(flow), _ptr(noise), _ptr(out), h, w, _stream(None)), name)
    return out


def temporal_loss(first, second, flow, out=None, warped_out=None, ws=None, valid=None):
    """mean |warp(first, flow) - second| per channel, a device float64 [3] tensor; uint8 frames count in units of 1 / 255, so both
    forms are on the 0..1 scale.  flow None: no warp (the reference's data_w=False).  warped_out (a frame like `first`): also
    receives warp(first, flow), the reference's second return value.  `out` and `ws` (uint8, at least workspace_bytes(h, w)
    bytes) are allocated when not given.

    valid (uint8 [h,w], uint8 frames only; vstnet_amd.flow.consistency): the means are taken over the pixels with valid != 0
    and the result is a float64 [4] tensor, the three means and the share of valid pixels (four zeros when there is none)."""
    import torch
    a, is_u8, h, w = _check_frame(first, "first")
    b = _check_like(_check_frame(second, "second")[0], a, "second")
    flow = _check_like(flow, a, "flow", (2, h, w), torch.float32)
    warped_out = _check_like(warped_out, a, "warped_out")
    dev = a.device
    need = workspace_bytes(h, w)
    n_out = 3
    if valid is not None:
        if not is_u8:
            raise ValueError("valid goes with uint8 frames")
        valid = _check_like(valid, a, "valid", (h, w), torch.uint8)
        n_out = 4
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n_out, dtype=torch.float64, device=dev)
        elif out.dtype != torch.float64 or out.numel() != n_out or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous float64 [{n_out}] tensor on {dev}")
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.device != dev:
            raise ValueError(f"ws must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
        if valid is not None:
            _lib.check(_lib.lib().vst_temporal_l1_masked_u8(_ptr(a), _ptr(b), _ptr(flow), _ptr(valid), h, w, _ptr(out),
                                                            _ptr(warped_out), _ptr(ws), _stream(None)),
                       "vst_temporal_l1_masked_u8")
            return out
        name = "vst_temporal_l1_u8" if is_u8 else "vst_temporal_l1_f32"
        _lib.check(getattr(_lib.lib(), name)(_ptr(a), _ptr(b), _ptr(flow), h, w, _ptr(out), _ptr(warped_out), _ptr(ws),
                                             _stream(None)), name)
    return out


class TemporalLoss:
    """The temporal loss of frames of ONE size with every buffer made up front: the three values and the workspace belong to
    this object, so one object serves one frame at a time (a pipeline keeps one per ring slot, like matting.MattingLoss).  Calls
    with an `out` of their own may follow one another on one stream: the workspace is free again when a call's second launch
    has run."""

    def __init__(self, hw, device=None):
        import torch
        self.hw = (int(hw[0]), int(hw[1]))
        self.device = _device(device)
        need = workspace_bytes(self.hw[0], self.hw[1])
        with torch.cuda.device(self.device):
            self.loss4 = torch.empty(4, dtype=torch.float64, device=self.device)    # with a mask: the means and the share
            self.loss = self.loss4[:3]
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)

    def __call__(self, first, second, flow, out=None, warped_out=None, valid=None):
        """-> the float64 [3] tensor, or with `valid` the float64 [4] one (this object's, or `out`); queued on the current
        stream."""
        _, _, h, w = _check_frame(first, "first")
        if (h, w) != self.hw:
            raise ValueError(f"made for {self.hw} frames, got {(h, w)}")
        if out is None:
            out = self.loss if valid is None else self.loss4
        return temporal_loss(first, second, flow, out=out, warped_out=warped_out, ws=self.ws, valid=valid)


def draw_fake_flow(hw, rng, motion_level=8, shift_level=10, cell=100):
    """The host-side draws of one fake flow from a numpy.random.Generator, in a fixed order: the coarse grid [h // cell,
    w // cell, 2] of normal(0, motion_level) values (x first), then the x shift and the y shift, whole numbers in -shift_level ..
    shift_level."""
    h, w = int(hw[0]), int(hw[1])
    if cell < 1 or h // cell < 1 or w // cell < 1:
        raise ValueError(f"a {w}x{h} frame has no coarse grid of {cell}-pixel cells: the frame must be at least one cell each way")
    grid = rng.normal(0.0, float(motion_level), size=(h // cell, w // cell, 2))
    sx, sy = (int(rng.integers(-int(shift_level), int(shift_level) + 1)) for _ in range(2))
    return grid, (sx, sy)


def fake_flow_from(grid, shifts, hw, ksize=100, device=None, out=None):
    """vst_fake_flow on draws the caller made: grid [gh,gw,2] (float64 or float32, host), shifts (x, y) -> float32 [2,h,w] on the
    card."""
    import torch
    h, w = int(hw[0]), int(hw[1])
    g = np.ascontiguousarray(np.asarray(grid), dtype=np.float64)
    if g.ndim != 3 or g.shape[2] != 2:
        raise ValueError(f"the coarse grid must be [gh,gw,2], got {g.shape}")
    gh, gw = int(g.shape[0]), int(g.shape[1])
    device = _device(device)
    if device.type != "cuda":
        raise ValueError("fake_flow makes the flow on the GPU (no CPU fallback)")
    need = fake_flow_workspace_bytes(h, w, gh, gw, ksize)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty((2, h, w), dtype=torch.float32, device=device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (2, h, w) or not out.is_contiguous() or out.device != device:
            raise ValueError(f"out must be a contiguous float32 [2,{h},{w}] tensor on {device}")
        d_grid = torch.from_numpy(g).to(device)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().vst_fake_flow(_ptr(d_grid), gh, gw, float(shifts[0]), float(shifts[1]), int(ksize), _ptr(out), h, w,
                                            _ptr(ws), _stream(None)), "vst_fake_flow")
    return out


def fake_flow(hw, rng, motion_level=8, shift_level=10, cell=100, ksize=100, device=None, out=None):
    """The reference's GenerateFakeFlow(h, w) as float32 [2,h,w] on the card.  motion_level > 0: a coarse grid of normal draws
    (one per `cell` pixels) upsampled bilinearly, a whole-number shift per axis, a ksize x ksize box blur - the draws come from
    `rng` (draw_fake_flow), everything else runs on the card.  motion_level = 0: the two shifts alone, as a constant flow (the
    reference allocates that one with its two sizes transposed; not copied).  `out`: the tensor to fill."""
    import torch
    h, w = int(hw[0]), int(hw[1])
    device = _device(device)
    if device.type != "cuda":
        raise ValueError("fake_flow makes the flow on the GPU (no CPU fallback)")
    if motion_level > 0:
        grid, shifts = draw_fake_flow((h, w), rng, motion_level, shift_level, cell)
        return fake_flow_from(grid, shifts, (h, w), ksize, device, out=out)
    sx, sy = (int(rng.integers(-int(shift_level), int(shift_level) + 1)) for _ in range(2))
    flow = out if out is not None else torch.empty((2, h, w), dtype=torch.float32, device=device)
    if flow.dtype != torch.float32 or tuple(flow.shape) != (2, h, w) or flow.device != device:
        raise ValueError(f"out must be a float32 [2,{h},{w}] tensor on {device}")
    flow[0].fill_(float(sx))
    flow[1].fill_(float(sy))
    return flow


def noise_plane(hw, level, seed, t, device):
    """Frame t's noise: level * torch.randn [3,h,w] from a device generator seeded from (seed, t)."""
    import torch
    gen = torch.Generator(device=device)
    gen.manual_seed((int(seed) * 1000003 + int(t)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randn((3, int(hw[0]), int(hw[1])), generator=gen, device=device, dtype=torch.float32) * float(level)


def synthetic_clip(still_u8, n_frames, seed=0, motion_level=8, shift_level=10, noise_level=0.001, device=None, cell=100,
                   ksize=100):
    """A clip with known motion from one still (uint8 [h,w,3], host array or tensor): the reference's GenerateFakeData chained.
    Frame 0 is the still; frame t = noise(warp(frame t-1, flow t)) with flow t a fake_flow and the noise a normal plane whose
    level is the one the reference's GaussianNoise uses, noise_level * (1 + u), u uniform in [0, 1).  All host draws (grid,
    shifts, u, in that order per frame) come from numpy.random.default_rng(seed); the noise plane from torch.randn with a device
    generator seeded from (seed, t).

    Returns (frames uint8 [n,h,w,3], flows float32 [n,2,h,w] with flows[0] unused (zeros), loss_in float64 [n] with loss_in[0] =
    nan), all on the card, queued on the current stream: loss_in[t] is the temporal loss of the INPUT pair, mean |warp(frame t-1,
    flow t) - frame t| - the noise alone, as rounded into uint8.

    The warp samples the nearest pixel and pads with the border, so every step repeats border pixels over what moved in and
    loses what moved out: chained over many frames the borders smear and the picture drifts away from the still.  Such clips are
    meant to be short (a handful of frames); they measure stability, they are not footage."""
    import torch
    device = _device(device)
    if device.type != "cuda":
        raise ValueError("synthetic_clip makes the clip on the GPU (no CPU fallback)")
    still = still_u8 if torch.is_tensor(still_u8) else torch.from_numpy(np.array(still_u8))
    if still.dtype != torch.uint8 or still.dim() != 3 or still.shape[2] != 3:
        raise ValueError(f"the still must be uint8 [h,w,3], got {still.dtype} {tuple(still.shape)}")
    n, (h, w) = int(n_frames), (int(still.shape[0]), int(still.shape[1]))
    if n < 1:
        raise ValueError("n_frames must be at least 1")
    rng = np.random.default_rng(int(seed))
    with torch.cuda.device(device):
        frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
        flows = torch.zeros((n, 2, h, w), dtype=torch.float32, device=device)
        loss3 = torch.full((n, 3), float("nan"), dtype=torch.float64, device=device)
        frames[0].copy_(still.to(device).contiguous())
        meter = TemporalLoss((h, w), device)
        for t in range(1, n):
            fake_flow((h, w), rng, motion_level, shift_level, cell, ksize, device, out=flows[t])
            level = float(noise_level) * (1.0 + float(rng.random()))
            warp(frames[t - 1], flows[t], noise_plane((h, w), level, seed, t, device), out=frames[t])
            meter(frames[t - 1], frames[t], flows[t], out=loss3[t])
        # mean3 on the card: the same two additions and one correctly rounded division.  The divisor is a tensor on purpose:
        # torch divides by a Python scalar as a multiplication by its reciprocal, which is an ulp off on one value in a few
        loss_in = (loss3[:, 0] + loss3[:, 1] + loss3[:, 2]) / torch.full((n,), 3.0, dtype=torch.float64, device=device)
    return frames, flows, loss_in
