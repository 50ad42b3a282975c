"""Temporal stabiliser on the device (csrc/stabilise.hip; DESIGN.md section 6, "Stabiliser"): the frame that is about to be written,
blended with the frame written before it sampled along the flow, where the input did not change along that flow.

With S = cur_out, q = p - flow(p), I~ = bilinear(prev_in; q) and O~ = bilinear(prev_written; q) on the 0..255 scale:

    e     = mean over the channels of (cur_in - I~)^2
    wgt   = gain / (1 + e / sigma^2)
    written = clamp(rint(S + clamp(wgt (O~ - S), -limit, limit)), 0, 255)

and written = S where q lies outside the frame, is not finite, or `valid` (vstnet_amd.flow.consistency) is 0.  Feeding each
frame's result back as the next frame's prev_written makes the filter recursive.  All arithmetic is fp64 and correctly rounded:
tests/stabilise_ref.py states it in numpy and the device gives the same bytes.

The defaults (gain 0.7, sigma 8 levels, limit 24 levels) are STARTING VALUES: they were tried in a numpy prototype on constructed
clips only.  Picture quality on real footage, with trained weights, is unmeasured, and so is the blur a long recursion may build up.

Frames are uint8 [h,w,3]; a flow is float32 [2,h,w], x displacement first, in the convention of vstnet_amd.temporal and
vstnet_amd.flow.  Every call is queued on the current stream and never waits for the card.  There is no CPU fallback: tensors off
the GPU raise ``ValueError``, arguments the kernel does not take raise ``VstError``.
"""
from __future__ import annotations

from . import _lib
from .resize import _ptr, _stream
from .temporal import _check_frame, _check_like, _device

DEFAULTS = {"gain": 0.7, "sigma": 8.0, "limit": 24.0}


def check_params(gain, sigma, limit):
    """(gain, sigma, limit) as floats, or ValueError: gain in (0, 1), sigma > 0 and finite, limit >= 0 and finite"""
    gain, sigma, limit = float(gain), float(sigma), float(limit)
    if not 0.0 < gain < 1.0:
        raise ValueError(f"the stabiliser's gain must be inside (0, 1), got {gain}")
    if not 0.0 < sigma < float("inf"):
        raise ValueError(f"the stabiliser's sigma must be above 0 (and finite), got {sigma}")
    if not 0.0 <= limit < float("inf"):
        raise ValueError(f"the stabiliser's limit must not be negative (and finite), got {limit}")
    return gain, sigma, limit


def stabilise(cur_in, prev_in, cur_out, prev_written, flow, valid=None, gain=DEFAULTS["gain"], sigma=DEFAULTS["sigma"],
              limit=DEFAULTS["limit"], out=None):
    """-> the frame to write, uint8 [h,w,3] (`out`, allocated when not given; never one of the inputs).  cur_in / prev_in: the
    encoder's input frames t and t-1; cur_out: the decoded frame t; prev_written: what this call returned for frame t-1; flow: the
    flow of (t, t-1); valid: uint8 [h,w] or None.  The defaults are starting values, unmeasured on real footage (module
    docstring)."""
    import torch
    a, is_u8, h, w = _check_frame(cur_in, "cur_in")
    if not is_u8:
        raise ValueError("the stabiliser works on uint8 [h,w,3] frames")
    frames = [_check_like(_check_frame(t, name)[0], a, name) for t, name in
              ((prev_in, "prev_in"), (cur_out, "cur_out"), (prev_written, "prev_written"))]
    flow = _check_like(flow, a, "flow", (2, h, w), torch.float32)
    if flow is None:
        raise ValueError("flow must be a float32 [2,h,w] tensor: a frame without a flow is written as it is")
    valid = _check_like(valid, a, "valid", (h, w), torch.uint8)
    gain, sigma, limit = check_params(gain, sigma, limit)
    with torch.cuda.device(a.device):
        if out is None:
            out = torch.empty_like(a)
        out = _check_like(out, a, "out")
        _lib.check(_lib.lib().vst_stabilise_u8(_ptr(a), _ptr(frames[0]), _ptr(frames[1]), _ptr(frames[2]), _ptr(flow), _ptr(valid),
                                               h, w, gain, sigma, limit, _ptr(out), _stream(None)), "vst_stabilise_u8")
    return out


class Stabiliser:
    """The stabiliser for frames of ONE size with its three parameters checked up front and one output frame of its own, so one
    object serves one frame at a time (a pipeline passes `out`, its history ring's slot).  Calls may follow one another on one
    stream; a call that passes this object's earlier result as prev_written needs an `out` of its own."""

    def __init__(self, hw, gain=DEFAULTS["gain"], sigma=DEFAULTS["sigma"], limit=DEFAULTS["limit"], device=None):
        import torch
        self.hw = (int(hw[0]), int(hw[1]))
        self.gain, self.sigma, self.limit = check_params(gain, sigma, limit)
        self.device = _device(device)
        if self.device.type != "cuda":
            raise ValueError("the stabiliser runs on the GPU (no CPU fallback)")
        with torch.cuda.device(self.device):
            self.written = torch.empty(self.hw + (3,), dtype=torch.uint8, device=self.device)

    def __call__(self, cur_in, prev_in, cur_out, prev_written, flow, valid=None, out=None):
        """-> the frame to write (this object's, or `out`); queued on the current stream."""
        _, _, h, w = _check_frame(cur_in, "cur_in")
        if (h, w) != self.hw:
            raise ValueError(f"made for {self.hw} frames, got {(h, w)}")
        return stabilise(cur_in, prev_in, cur_out, prev_written, flow, valid, self.gain, self.sigma, self.limit,
                         out=self.written if out is None else out)
