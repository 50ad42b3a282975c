"""The reference's import path for its temporal loss, on the device: ``warp`` and ``TemporalLoss`` with the reference's method
names, call sequence and return values (train.py: ``second, flow = loss.GenerateFakeData(first)``, later ``loss(styled_first,
styled_second, flow)``).  Tensors are float [B,3,H,W] on the GPU; what comes back has their dtype.  The warp, the noise, the L1 mean
and the fake flow run in vstnet_amd/temporal.py (csrc/temporal.hip).  The host draws come from the generators the reference uses,
in its order - ``np.random.normal`` for the coarse grid, two ``random.randint`` for the shifts, one ``random.random()`` for the
noise level - so seeding ``random`` and ``np.random`` fixes a run; the noise plane itself is ``torch.randn`` on the card.  Nothing
here needs OpenCV."""
import random

import numpy as np
import torch
import torch.nn as nn


def _frames(x, what):
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4 or x.shape[1] != 3 or not x.is_floating_point():
        raise ValueError(f"{what} must be a float [B,3,H,W] tensor on the GPU (no CPU fallback)")
    return x.detach().to(torch.float32).contiguous()


def _flows(flo, like):
    """the flow of every frame of `like`: [B,2,H,W], or [1,2,H,W] for all of them"""
    if not torch.is_tensor(flo) or flo.device != like.device or flo.dim() != 4 or flo.shape[1] != 2 \
            or tuple(flo.shape[2:]) != tuple(like.shape[2:]) or flo.shape[0] not in (1, like.shape[0]):
        raise ValueError(f"the flow must be a [B,2,H,W] tensor on {like.device} for frames {tuple(like.shape)}")
    flo = flo.detach().to(torch.float32).contiguous()
    return [flo[b if flo.shape[0] > 1 else 0] for b in range(like.shape[0])]


def _warp_each(xs, flows, level=None):
    """temporal.warp frame by frame (flows: one [2,H,W] per frame, or None), with a fresh normal plane of deviation `level`"""
    from vstnet_amd import temporal
    out = torch.empty_like(xs)
    for b in range(xs.shape[0]):
        noise = None if level is None else torch.randn_like(xs[b]) * level
        temporal.warp(xs[b], None if flows is None else flows[b], noise, out=out[b])
    return out


def warp(x, flo, padding_mode='border'):
    """x [B,3,H,W] sampled at (pixel - flo), nearest pixel, border padding: vstnet_amd.temporal.warp per frame."""
    if padding_mode != 'border':
        raise NotImplementedError("warp: only padding_mode='border' (what the reference's loss uses) is on the device")
    xs = _frames(x, "x")
    return _warp_each(xs, _flows(flo, xs)).to(x.dtype)


class TemporalLoss(nn.Module):
    """Flicker under made-up motion: a frame and its warped, noised twin should stylise to a pair that agrees after the same
    warp.  The keywords, attributes and methods are the reference's."""
    cell = 100          # the reference's coarse grid: one normal draw per 100 pixels
    ksize = 100         # and its box blur

    def __init__(self, data_sigma=True, data_w=True, noise_level=0.001, motion_level=8, shift_level=10):
        super().__init__()
        self.data_sigma, self.data_w = data_sigma, data_w
        self.noise_level, self.motion_level, self.shift_level = noise_level, motion_level, shift_level

    @staticmethod
    def _noise_level(stddev):
        """the deviation of one noise plane: between stddev and twice that, by one random.random() draw"""
        return stddev * (1.0 + random.random())

    def _shifts(self):
        """the whole-frame shift per axis, x then y: two random.randint draws"""
        lim = int(self.shift_level)
        return [random.randint(-lim, lim) for _ in range(2)]

    def GaussianNoise(self, ins, mean=0, stddev=0.001):
        return ins + (torch.randn_like(ins) * self._noise_level(stddev) + mean)

    def GenerateFakeFlow(self, height, width):
        """-> float32 [2,height,width] on the current GPU (the reference makes it on the host and moves it)"""
        from vstnet_amd import temporal
        dev = torch.device("cuda", torch.cuda.current_device())
        if self.motion_level > 0:
            gh, gw = height // self.cell, width // self.cell
            if gh < 1 or gw < 1:
                raise ValueError(f"a {width}x{height} frame has no coarse grid of {self.cell}-pixel cells")
            grid = np.random.normal(0.0, self.motion_level, (gh, gw, 2))
            return temporal.fake_flow_from(grid, self._shifts(), (height, width), self.ksize, dev)
        sx, sy = self._shifts()
        flow = torch.empty((2, height, width), dtype=torch.float32, device=dev)
        flow[0].fill_(float(sx))
        flow[1].fill_(float(sy))
        return flow

    def GenerateFakeData(self, first_frame):
        """first_frame [B,3,H,W] in 0..1 -> (second_frame, forward_flow [B,2,H,W] or None): one flow for the batch (data_w), one
        noise level for the batch and a plane per frame (data_sigma), warp and noise in one launch per frame."""
        xs = _frames(first_frame, "first_frame")
        B, _, H, W = xs.shape
        flow = self.GenerateFakeFlow(H, W).to(xs.device) if self.data_w else None
        level = self._noise_level(self.noise_level) if self.data_sigma else None
        second = _warp_each(xs, None if flow is None else [flow] * B, level)
        return second.to(first_frame.dtype), None if flow is None else flow[None].expand(B, 2, H, W)

    def forward(self, first_frame, second_frame, forward_flow):
        """-> (mean |warp(first, flow) - second|, the warped first frame), in the dtype of first_frame"""
        from vstnet_amd import temporal
        a, b = _frames(first_frame, "first_frame"), _frames(second_frame, "second_frame")
        if a.shape != b.shape:
            raise ValueError(f"the two frames differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
        flows = _flows(forward_flow, a) if self.data_w else None
        warped = torch.empty_like(a) if self.data_w else None
        loss3 = torch.empty((a.shape[0], 3), dtype=torch.float64, device=a.device)
        for k in range(a.shape[0]):
            temporal.temporal_loss(a[k], b[k], None if flows is None else flows[k], out=loss3[k],
                                   warped_out=None if warped is None else warped[k])
        return loss3.mean().to(first_frame.dtype), (first_frame if warped is None else warped.to(first_frame.dtype))
