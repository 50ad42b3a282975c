"""RevResNet — drop-in for the reference's ``models.RevResNet.RevResNet`` on MI355X.

Same constructor, attributes, call convention and state_dict keys as the reference
(models/RevResNet.py:166-239): ``net(x, forward=True)`` encodes ``x[B,3,H,W]`` to
``z[B,32,H,W]`` (photorealistic: hidden_dim=16, sp_steps=2) or ``z[B,128,H/2,W/2]`` (artistic: 64, 1);
``net(z, forward=False)`` is the exact inverse with recomputed activations.  All device work goes
through the C ABI of ``libvstnet_hip.so`` (include/vstnet.h); there is no CPU or torch-op fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .code import PackedCode
from .synth import CONV_IDX

_PRECISIONS = _lib.PRECISIONS


def _stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_frame(H, W, what="H and W"):
    """The whole-frame passes' shape rule (vst_shape_ok): multiples of 4, >= 8, and at most VST_MAX_FRAME_PIXELS pixels."""
    if H % 4 or W % 4 or H < 8 or W < 8:
        raise RuntimeError(f"{what} must be multiples of 4 and >= 8 (got {H}x{W})")
    limit = int(_lib.lib().vst_max_frame_pixels())
    if H * W > limit:
        raise RuntimeError(f"a {H}x{W} frame is past the whole-frame limit of {limit} pixels (include/vstnet.h "
                           "VST_MAX_FRAME_PIXELS): stylise it in halo tiles with vstnet_amd.tiled.stylize_tiled")


class residual_block(nn.Module):
    """Parameter container with the reference's layout (models/RevResNet.py:68-94): ``conv`` is a
    Sequential whose entries 1, 4, 7 are the three 3x3 convolutions (the others are placeholders
    for ReflectionPad2d / ReLU, which the HIP kernels fuse)."""

    def __init__(self, channel, stride=1, mult=4, kernel=3):
        super().__init__()
        self.stride = stride
        self.channel = channel
        in_ch = channel if stride == 1 else channel // 4
        mid = channel // mult
        self.conv = nn.Sequential(
            nn.Identity(), nn.Conv2d(in_ch, mid, kernel, stride=stride, padding=0, bias=True), nn.Identity(),
            nn.Identity(), nn.Conv2d(mid, mid, kernel, padding=0, bias=True), nn.Identity(),
            nn.Identity(), nn.Conv2d(mid, channel, kernel, padding=0, bias=True),
        )
        for m in self.conv:                       # reference init_layers(): zero biases
            if isinstance(m, nn.Conv2d):
                m.bias.data.zero_()


class channel_reduction(nn.Module):
    """models/RevResNet.py:119-129 (pad = out_ch*4**sp_steps - in_ch must be 0, as in both modes)."""

    def __init__(self, in_ch, out_ch, sp_steps=2, n_blocks=2, kernel=3):
        super().__init__()
        self.pad = out_ch * 4 ** sp_steps - in_ch
        self.sp_steps = sp_steps
        self.n_blocks = n_blocks
        self.block_list = nn.ModuleList(
            [residual_block(out_ch * 4 ** sp_steps, stride=1, mult=4, kernel=kernel) for _ in range(n_blocks)])


class RevResNet(nn.Module):
    def __init__(self, nBlocks=[10, 10, 10], nStrides=[1, 2, 2], nChannels=[16, 64, 256], in_channel=3, mult=4,
                 hidden_dim=16, sp_steps=2, kernel=3, precision=None):
        super().__init__()
        if not nChannels:                                    # models/RevResNet.py:179-180
            nChannels = [in_channel * 2, in_channel * 2 * 4, in_channel * 2 * 4 ** 2]
        nBlocks, nStrides, nChannels = list(nBlocks), list(nStrides), list(nChannels)
        # The tuned kernels (conv.hip / conv3.hip, ZC layout, packed code) implement the published CAP-VSTNet architecture; every
        # other constructor argument set the reference accepts runs on the generic HIP ops (csrc/generic.hip, vstnet_amd/generic.py):
        # exact fp32, NCHW, complete but slow.
        self._generic = not ((nBlocks, nStrides, nChannels, mult, kernel) == ([10, 10, 10], [1, 2, 2], [16, 64, 256], 4, 3)
                             and sp_steps in (1, 2) and hidden_dim * 4 ** sp_steps == 256 and 1 <= in_channel <= 16)
        if self._generic:
            if not (len(nBlocks) == len(nStrides) == len(nChannels) and len(nBlocks) >= 1 and all(b >= 1 for b in nBlocks)):
                raise ValueError("nBlocks, nStrides and nChannels need the same length and at least one block per stage")
            if any(s not in (1, 2) for s in nStrides) or kernel % 2 == 0 or not (1 <= kernel <= 7):
                raise NotImplementedError("generic path: strides in {1, 2}, odd kernel <= 7")
            if nStrides[0] == 2:
                raise NotImplementedError("generic path: the first stage must have stride 1 (as in the reference's defaults)")
            prev = nChannels[0]
            for i, (ch, st) in enumerate(zip(nChannels, nStrides)):
                want = prev * 4 if st == 2 else prev
                if ch != want:
                    raise ValueError(f"stage {i}: {ch} channels cannot follow {prev} with stride {st} (a stride-2 block squeezes "
                                     "its halves: x4 channels; a stride-1 stage keeps them)")
                if ch // mult < 1:      # (the reference floors: channel // mult, models/RevResNet.py:81 - no divisibility needed)
                    raise ValueError(f"stage {i}: channel {ch} // mult {mult} leaves no intermediate channel")
                prev = ch
            if hidden_dim * 4 ** sp_steps < nChannels[-1] or 2 * nChannels[0] < in_channel:
                raise ValueError("channel_reduction pad = hidden_dim * 4**sp_steps - nChannels[-1] and the input pad "
                                 "2 * nChannels[0] - in_channel must be >= 0")
        self.nBlocks = nBlocks
        self.in_channel = in_channel
        self.pad = 2 * nChannels[0] - in_channel
        self.in_ch = nChannels[0]
        self.down_scale = np.prod(np.array(nStrides))
        self.hidden_dim = hidden_dim
        self.sp_steps = sp_steps
        strides, chans = [], []
        for ch, depth, st in zip(nChannels, nBlocks, nStrides):     # block_stack, models/RevResNet.py:190-201
            strides += [st] + [1] * (depth - 1)
            chans += [ch] * depth
        self.stack = nn.ModuleList([residual_block(ch, st, mult=mult, kernel=kernel) for ch, st in zip(chans, strides)])
        self.channel_reduction = channel_reduction(nChannels[-1], hidden_dim, sp_steps=sp_steps, kernel=kernel)
        precision = precision or _lib.default_precision()
        if precision not in _PRECISIONS and precision != "auto":
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS) + ['auto']}")
        # "auto": the fastest of f16x2h / f16x2 / bf16x3 that a probe stylisation on THIS checkpoint keeps within
        # `auto_tolerance` of the bf16x3 result (see _auto_select); decided after every (re)pack, readable as
        # resolved_precision / calibration
        self.precision = precision
        self.auto_tolerance = 2.5e-4
        self.resolved_precision = None if precision == "auto" else precision
        self.calibration = None
        # photorealistic mode: net(x) returns the code as a PackedCode (code.py: [B,32,H,W] to every caller, kept in the
        # coupling blocks' own layout for cWCT and the inverse pass) where the passes run image by image anyway (_use_packed);
        # "always": for every batch; False or VST_PACKED_CODE=0: always plain NCHW
        self.packed_code = os.environ.get("VST_PACKED_CODE", "1") != "0"
        # exponent normalisation of h1 / h2 at pack time (function-preserving, exact in fp32; see vst_normalize_block)
        self.normalize_intermediates = os.environ.get("VST_NORMALIZE", "1") != "0"
        # fp16 modes: probe pass + range flags after every (re)pack (see _calibrate)
        self.calibrate_on_load = os.environ.get("VST_CALIBRATE", "1") != "0"
        self._packed = None          # (device, blob tensor, bias tensors, NetWeights struct, parameter versions)
        self._workspace = None
        # a PARENT module's load_state_dict never calls this module's load_state_dict: invalidate through the hook as well
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module._invalidate())

    # ------------------------------------------------------------------ weight packing
    def _blocks(self):
        return list(self.stack) + list(self.channel_reduction.block_list)

    def _invalidate(self):
        self._packed = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._invalidate()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate()
        return out

    def refresh_weights(self):
        """Drop the packed weight copies (rebuilt on the next call).  Needed only after edits the cache key cannot see:
        writes through ``param.data`` (``p.data.copy_(...)``); in-place ops on the parameter itself, ``load_state_dict``
        and ``.to()`` are noticed automatically."""
        self._invalidate()

    def _param_versions(self, convs):
        # in-place edits of the PARAMETER (p.copy_ / p.add_ under no_grad, optimizer.step, load_state_dict's copy_) bump its
        # _version.  Edits through `p.data` do NOT (p.data is a separate tensor object with its own counter and the same
        # storage): after p.data.copy_(...) call refresh_weights().
        return tuple(p._version for c in convs for p in (c.weight, c.bias)) + tuple(p.data_ptr() for c in convs for p in (c.weight, c.bias))

    def _ensure_packed(self, device):
        convs = []
        for blk in self._blocks():
            for ci in CONV_IDX:
                convs.append(blk.conv[ci])
        versions = self._param_versions(convs)
        if self._packed is not None and self._packed[0] == device and self._packed[4] == versions:
            return self._packed[3]
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()) and self.training:
            raise RuntimeError("vstnet_amd.RevResNet is an inference path (its outputs carry no autograd graph): call "
                               ".eval() or run under torch.no_grad()")
        L = _lib.lib()
        sizes = [L.vst_conv_packed_bytes(c.out_channels, c.in_channels) for c in convs]
        offsets = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in sizes])])
        blob = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=device)
        biases = []
        net = _lib.NetWeights()
        with torch.cuda.device(device):
            st = _stream_ptr()
            wb = []
            for c in convs:
                if c.weight.device != device:
                    raise RuntimeError(f"RevResNet parameters live on {c.weight.device}, input on {device}: call .to(device)")
                # copies: the packed weights and their bias age together, and the normalisation below works in place
                wb.append((c.weight.detach().to(torch.float32).clone(memory_format=torch.contiguous_format),
                           c.bias.detach().to(torch.float32).clone()))
            if self.normalize_intermediates:     # vstnet.h vst_normalize_block: h1 / h2 channels to unit weight-row scale
                for j in range(0, len(convs), 3):
                    (w1, b1), (w4, b4), (w7, _) = wb[j:j + 3]
                    _lib.check(L.vst_normalize_block(C.c_void_p(w1.data_ptr()), C.c_void_p(b1.data_ptr()), C.c_void_p(w4.data_ptr()),
                                                     C.c_void_p(b4.data_ptr()), C.c_void_p(w7.data_ptr()), convs[j].in_channels,
                                                     convs[j].out_channels, convs[j + 2].out_channels, C.c_void_p(0), st),
                               "vst_normalize_block")
            for k, c in enumerate(convs):
                w, b = wb[k]
                biases.append((w, b))
                _lib.check(L.vst_pack_conv(C.c_void_p(w.data_ptr()), c.out_channels, c.in_channels,
                                           C.c_void_p(blob.data_ptr() + int(offsets[k])), st), "vst_pack_conv")
                cw = net.blocks[k // 3].conv[k % 3]
                cw.packed = blob.data_ptr() + int(offsets[k])
                cw.bias = b.data_ptr()
            # one-off: the packed blob may be used from any stream afterwards (frames in flight on several streams)
            torch.cuda.current_stream(device).synchronize()
        self._packed = (device, blob, biases, net, versions)
        if self.precision == "auto":
            self._auto_select(device)
        elif self.precision in ("f16x2", "f16x2h") and self.calibrate_on_load:
            self._calibrate(device)
        return net

    def _prec(self):
        """C-ABI code of the arithmetic the passes run in (the resolved mode under precision='auto')."""
        return _PRECISIONS[self.resolved_precision or "bf16x3"]

    # ------------------------------------------------------------------ precision="auto"
    def calibrate(self, content=None, style=None):
        """precision='auto': (re)decide the arithmetic mode on sample frames of the caller's own data ([1,3,H,W] in the
        caller's value range; default: two seeded uniform [0,1) 128x128 frames).  Returns the calibration record."""
        if self.precision != "auto":
            raise RuntimeError("calibrate() chooses a mode for precision='auto'; this module's precision is fixed")
        dev = next(self.parameters()).device
        self._ensure_packed(dev)
        return self._auto_select(dev, content, style)

    def _auto_select(self, device, content=None, style=None):
        """One probe stylisation (encode content + style, cWCT, decode) per candidate mode, compared ON THE DEVICE with the same
        probe in bf16x3, the fp32-class mode: a candidate is taken if its codes and its stylised frame are within
        `auto_tolerance` (rel-L2; default 2.5e-4, a quarter of the 1e-3 budget) and the worst channel of z_cs within 10x that,
        and no fp16 range flag was raised.  Fastest first: f16x2h, f16x2; otherwise bf16x3.  The narrowed modes' error is a
        property of the checkpoint (11-bit weights are a fixed perturbation of the model; how much the model amplifies it is
        what this measures), so one probe per (re)pack decides; calibrate() repeats it on the caller's own frames."""
        from .cwct import cWCT
        from .synth import synthetic_frames
        xc = synthetic_frames(1, 128, 128, seed=4242).to(device) if content is None else content.to(device)
        xs = synthetic_frames(1, 128, 128, seed=4243).to(device) if style is None else style.to(device)
        cw = cWCT(precision="bf16x3")
        rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))       # noqa: E731

        def probe(mode):
            self.resolved_precision = mode
            _lib.range_flags(reset=True)
            zc = self(xc)
            zcs = cw.transfer(zc, self(xs))
            out = self(zcs, forward=False)
            dense = lambda t: t.materialize() if isinstance(t, PackedCode) else t                    # noqa: E731
            return dense(zc), dense(zcs), out, _lib.range_flags(reset=True)

        record = {"tolerance": self.auto_tolerance, "candidates": {}}
        with torch.cuda.device(device), torch.no_grad():
            r_zc, r_zcs, r_out, _ = probe("bf16x3")
            chosen = "bf16x3"
            for mode in ("f16x2h", "f16x2"):
                zc, zcs, out, flags = probe(mode)
                d = (zcs.double() - r_zcs.double()).transpose(0, 1).reshape(zcs.shape[1], -1).norm(dim=1)
                n = r_zcs.double().transpose(0, 1).reshape(zcs.shape[1], -1).norm(dim=1)
                errs = {"z_c": rel(zc, r_zc), "z_cs": rel(zcs, r_zcs), "stylized": rel(out, r_out),
                        "z_cs_worst_channel": float((d / (n + 1e-300)).max()), "range_flags": int(flags)}
                ok = (flags == 0 and max(errs["z_c"], errs["z_cs"], errs["stylized"]) <= self.auto_tolerance
                      and errs["z_cs_worst_channel"] <= 10 * self.auto_tolerance)
                errs["accepted"] = bool(ok)
                record["candidates"][mode] = errs
                if ok:
                    chosen = mode
                    break
        self.resolved_precision = record["chosen"] = chosen
        self.calibration = record
        return record

    # ------------------------------------------------------------------ fp16 range (the narrowed modes only)
    def check_range(self, sample=None):
        """One forward + inverse pass of ``sample`` ([B,3,H,W] in the caller's value range; default: a seeded uniform [0,1)
        64x64 frame) and the fp16 range flags it raised on the device (vstnet.h VST_RANGE_*: 1 = an activation beyond
        +-65504 was clamped, 2 = a weight beyond fp16 range).  0 = the fp16 modes saw nothing out of range.  The flags are
        device-wide and sticky; this call clears them before and after (it synchronises the device: a calibration call)."""
        from .synth import synthetic_frames
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("vstnet_amd.RevResNet runs on ROCm devices only (no CPU fallback): move the module to 'cuda'")
        x = synthetic_frames(1, 64, 64, seed=12345).to(dev) if sample is None else sample.to(dev)
        with torch.cuda.device(dev), torch.no_grad():
            _lib.range_flags(reset=True)
            z = self(x)
            self(z, forward=False)
            return _lib.range_flags(reset=True)

    def _calibrate(self, device):
        """Load-time check of the fp16 modes (after every repack): the packed fp16 weights must be finite and a probe frame
        must pass without saturating an fp16 operand; otherwise the mode is unusable on this checkpoint and says so."""
        with torch.cuda.device(device):
            flags = _lib.range_flags(reset=True) & _lib.RANGE_WEIGHT       # raised by vst_pack_conv just now
        if not flags:
            flags = self.check_range()
        if flags:
            self._packed = None
            what = []
            if flags & _lib.RANGE_WEIGHT:
                what.append("a conv weight is beyond the fp16 range")
            if flags & _lib.RANGE_SATURATED:
                what.append("an activation of the probe frame saturated at +-65504")
            raise RuntimeError(f"precision='{self.precision}' cannot represent this checkpoint ({'; '.join(what)}): "
                               "use precision='bf16x3'")

    def _get_workspace(self, nbytes, device):
        """Pass workspace, one per (device, stream): frames in flight on different streams must not share state."""
        if self._workspace is None:
            self._workspace = {}
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        ws = self._workspace.get(key)
        if ws is None or ws.numel() < nbytes:
            self._workspace[key] = ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    # ------------------------------------------------------------------ the reference's call surface
    def forward(self, x, forward=True):
        return self._forward(x) if forward else self._inverse(x)

    def _check(self, t, channels, what):
        if not t.is_cuda:
            raise RuntimeError("vstnet_amd.RevResNet runs on ROCm devices only (no CPU fallback): move the "
                               "module and its inputs to 'cuda'")
        if t.dim() != 4 or t.shape[1] != channels:
            raise RuntimeError(f"{what}: expected [B,{channels},H,W], got {tuple(t.shape)}")
        return t.detach().to(torch.float32).contiguous()

    def _generic_params_ready(self, device):
        for p in self.parameters():
            if p.device != device or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"generic-architecture RevResNet: parameters must be contiguous float32 on {device} "
                                   f"(found {p.dtype} on {p.device}): call .float().to(device)")

    def _forward(self, x):
        """models/RevResNet.py:210-223."""
        x = self._check(x, self.in_channel, "RevResNet forward input")
        if self._generic:
            from . import generic
            ds = int(self.down_scale)
            if x.shape[2] % ds or x.shape[3] % ds:
                raise RuntimeError(f"H and W must be multiples of down_scale = {ds} (got {x.shape[2]}x{x.shape[3]})")
            self._generic_params_ready(x.device)
            with torch.cuda.device(x.device), torch.no_grad():
                return generic.forward(self, x)
        B, _, H, W = x.shape
        _check_frame(H, W)
        L = _lib.lib()
        net = self._ensure_packed(x.device)
        s = self.sp_steps
        if self._use_packed(B, H, W):            # the code stays in the coupling blocks' layout (code.py)
            code = torch.empty((B, 32 * H * W), dtype=torch.float32, device=x.device)
            ws = self._get_workspace(L.vst_pass_workspace_bytes(1, H, W), x.device)
            with torch.cuda.device(x.device):
                _lib.check(L.vst_revnet_encode(C.byref(net), C.c_void_p(x.data_ptr()), C.c_void_p(code.data_ptr()),
                                               C.c_void_p(ws.data_ptr()), B, self.in_channel, H, W,
                                               self._prec(), _stream_ptr()), "vst_revnet_encode")
            return PackedCode(code, H, W, None, None, s)
        z = torch.empty((B, 32, H, W) if s == 2 else (B, 128, H // 2, W // 2), dtype=torch.float32, device=x.device)
        ws = self._get_workspace(L.vst_pass_workspace_bytes(B, H, W), x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.vst_revnet_forward(C.byref(net), C.c_void_p(x.data_ptr()), C.c_void_p(z.data_ptr()),
                                            C.c_void_p(ws.data_ptr()), B, self.in_channel, H, W, s,
                                            self._prec(), _stream_ptr()), "vst_revnet_forward")
        return z

    def _float_out(self, out, B, H, W, device):
        """The float destination of an inverse pass: a new tensor, or the caller's [B,C,H,W] fp32 buffer."""
        shape = (B, self.in_channel, H, W)
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=device)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
            raise ValueError(f"scratch must be a contiguous fp32 tensor of shape {shape} on {device}")
        return out

    def _inverse(self, z, out=None):
        """models/RevResNet.py:225-239.  out: the caller's destination instead of a new tensor (the published architecture)."""
        s = self.sp_steps
        if self._generic:
            from . import generic
            z = self._check(z, 2 * self.hidden_dim, "RevResNet inverse input")
            if z.shape[2] % (2 ** s) or z.shape[3] % (2 ** s):
                raise RuntimeError(f"code height / width must be multiples of {2 ** s}")
            self._generic_params_ready(z.device)
            with torch.cuda.device(z.device), torch.no_grad():
                return generic.inverse(self, z)
        if isinstance(z, PackedCode) and z.sp_steps == s and not z.stale:
            return self._decode_packed(z, u8=False, out=out)
        z = self._check(z, 32 if s == 2 else 128, "RevResNet inverse input")
        B = z.shape[0]
        H, W = (z.shape[2], z.shape[3]) if s == 2 else (z.shape[2] * 2, z.shape[3] * 2)
        _check_frame(H, W, "the code's frame H and W")
        L = _lib.lib()
        net = self._ensure_packed(z.device)
        x = self._float_out(out, B, H, W, z.device)
        ws = self._get_workspace(L.vst_pass_workspace_bytes(B, H, W), z.device)
        with torch.cuda.device(z.device):
            _lib.check(L.vst_revnet_inverse(C.byref(net), C.c_void_p(z.data_ptr()), C.c_void_p(x.data_ptr()),
                                            C.c_void_p(ws.data_ptr()), B, self.in_channel, H, W, s,
                                            self._prec(), _stream_ptr()), "vst_revnet_inverse")
        return x

    def _use_packed(self, B, H, W):
        """The packed passes run one image at a time (an image's two state halves are adjacent in the code).  That is what
        the dense passes do anyway once an image's working set reaches their cache budget (vst_pass_sub_batch == 1);
        batches of SMALL images keep the dense route, whose launches cover several images."""
        if self.packed_code == "always":
            return True
        return bool(self.packed_code) and (B == 1 or _lib.lib().vst_pass_sub_batch(B, H, W) == 1)

    def _decode_packed(self, z, u8, out=None):
        """Inverse pass straight from the packed rows; a pending cWCT affine map is applied while the state is loaded.
        out (float form only): the caller's destination instead of a new tensor."""
        code, aff, lab, st, mix = z.packed, z.pending_affines, z.pending_labels, z.pending_strength, z.pending_mix
        if not code.is_cuda:
            raise RuntimeError("vstnet_amd.RevResNet runs on ROCm devices only (no CPU fallback)")
        B = code.shape[0]
        H, W = z.image_hw
        L = _lib.lib()
        net = self._ensure_packed(code.device)
        out = (torch.empty((B, H, W, 3), dtype=torch.uint8, device=code.device) if u8
               else self._float_out(out, B, H, W, code.device))
        if u8 and self.in_channel != 3:
            raise RuntimeError("inverse_u8 needs in_channel == 3")
        ws = self._get_workspace(L.vst_pass_workspace_bytes(1, H, W), code.device)
        aptr = C.c_void_p(aff.data_ptr()) if aff is not None else C.c_void_p(0)
        with torch.cuda.device(code.device):
            if lab is not None:                  # a masked cWCT is pending: one decode per image, a map per row
                per_image, ms = lab
                prec = self._prec()
                for b in range(B):
                    a_b, rows_b, plan_b = per_image[b]
                    blend = () if st is None else (C.c_void_p(st[b].data_ptr()),)      # a strength map: the _blend calls
                    args = (C.byref(net), C.c_void_p(code[b].data_ptr()), C.c_void_p(a_b.data_ptr()), C.c_void_p(rows_b.data_ptr()),
                            C.c_void_p(plan_b.data_ptr()), ms, *blend, C.c_void_p(out[b].data_ptr()), C.c_void_p(ws.data_ptr()))
                    fn = "vst_revnet_decode_labels" + ("_blend" if st is not None else "") + ("_u8" if u8 else "")
                    if u8:
                        _lib.check(getattr(L, fn)(*args, H, W, prec, _stream_ptr()), fn)
                    else:
                        _lib.check(getattr(L, fn)(*args, self.in_channel, H, W, prec, _stream_ptr()), fn)
                return out
            blend = () if st is None else (C.c_void_p(st.data_ptr()),)
            fn = "vst_revnet_decode" + ("_blend" if st is not None else "") + ("_u8" if u8 else "")
            if mix is not None:                  # a style map: K maps per image and a weight per row and map, the _mix calls
                fn = "vst_revnet_decode_mix" + ("_u8" if u8 else "")
                blend = (mix.shape[1], C.c_void_p(mix.data_ptr()), C.c_void_p(st.data_ptr() if st is not None else 0))
            if u8:
                _lib.check(getattr(L, fn)(C.byref(net), C.c_void_p(code.data_ptr()), aptr, *blend, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(ws.data_ptr()), B, H, W, self.sp_steps, self._prec(), _stream_ptr()), fn)
            else:
                _lib.check(getattr(L, fn)(C.byref(net), C.c_void_p(code.data_ptr()), aptr, *blend, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(ws.data_ptr()), B, self.in_channel, H, W, self.sp_steps,
                                          self._prec(), _stream_ptr()), fn)
        return out

    # ------------------------------------------------------------------ uint8 frame edge
    def forward_u8(self, frames):
        """Encode uint8 HWC frames [B,H,W,3] (what PIL / cv2 hand over) — ToTensor's u8/255 scaling and the
        HWC->planes transpose happen inside the first boundary kernel (image_transfer.py:167, video_transfer.py:188)."""
        if self._generic:
            raise NotImplementedError("the uint8 frame edge exists for the published architecture only")
        if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise RuntimeError("forward_u8 expects a CUDA uint8 tensor [B,H,W,3]")
        if self.in_channel != 3:
            raise RuntimeError("forward_u8 needs in_channel == 3")
        frames = frames.contiguous()
        B, H, W, _ = frames.shape
        _check_frame(H, W)
        L = _lib.lib()
        net = self._ensure_packed(frames.device)
        s = self.sp_steps
        if self._use_packed(B, H, W):
            code = torch.empty((B, 32 * H * W), dtype=torch.float32, device=frames.device)
            ws = self._get_workspace(L.vst_pass_workspace_bytes(1, H, W), frames.device)
            with torch.cuda.device(frames.device):
                _lib.check(L.vst_revnet_encode_u8(C.byref(net), C.c_void_p(frames.data_ptr()), C.c_void_p(code.data_ptr()),
                                                  C.c_void_p(ws.data_ptr()), B, H, W, self._prec(),
                                                  _stream_ptr()), "vst_revnet_encode_u8")
            return PackedCode(code, H, W, None, None, s)
        z = torch.empty((B, 32, H, W) if s == 2 else (B, 128, H // 2, W // 2), dtype=torch.float32, device=frames.device)
        ws = self._get_workspace(L.vst_pass_workspace_bytes(B, H, W), frames.device)
        with torch.cuda.device(frames.device):
            _lib.check(L.vst_revnet_forward_u8(C.byref(net), C.c_void_p(frames.data_ptr()), C.c_void_p(z.data_ptr()),
                                               C.c_void_p(ws.data_ptr()), B, H, W, s, self._prec(),
                                               _stream_ptr()), "vst_revnet_forward_u8")
        return z

    def inverse_u8(self, z, luminance_of=None, scratch=None):
        """Decode a code to uint8 HWC frames with the reference's quantisation: mul(255).clamp(0,255).byte()
        (truncation; image_transfer.py:217-218, video_transfer.py:212) fused into the last boundary kernel.
        luminance_of: the uint8 [B,H,W,3] device frames whose Lab luminance the result keeps (the fork's post-process,
        vstnet_amd/color.py): the code - in any form net(z, forward=False) takes - is decoded to float planes into `scratch`
        (a caller-owned contiguous [B,3,H,W] fp32 buffer; allocated per call if None) and one pointwise launch blends and
        quantises it into the uint8 result.  Without it nothing changes."""
        s = self.sp_steps
        if self._generic:
            raise NotImplementedError("the uint8 frame edge exists for the published architecture only")
        if luminance_of is not None:
            from .color import luminance_transfer_u8
            if self.in_channel != 3:
                raise RuntimeError("inverse_u8 needs in_channel == 3")
            return luminance_transfer_u8(luminance_of, self._inverse(z, out=scratch))
        if scratch is not None:
            raise ValueError("scratch is the float staging of luminance_of; without it the pass writes the uint8 frame directly")
        if isinstance(z, PackedCode) and z.sp_steps == s and not z.stale:
            return self._decode_packed(z, u8=True)
        z = self._check(z, 32 if s == 2 else 128, "RevResNet inverse input")
        B = z.shape[0]
        H, W = (z.shape[2], z.shape[3]) if s == 2 else (z.shape[2] * 2, z.shape[3] * 2)
        _check_frame(H, W, "the code's frame H and W")
        L = _lib.lib()
        net = self._ensure_packed(z.device)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=z.device)
        ws = self._get_workspace(L.vst_pass_workspace_bytes(B, H, W), z.device)
        with torch.cuda.device(z.device):
            _lib.check(L.vst_revnet_inverse_u8(C.byref(net), C.c_void_p(z.data_ptr()), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(ws.data_ptr()), B, H, W, s, self._prec(),
                                               _stream_ptr()), "vst_revnet_inverse_u8")
        return out

    @torch.no_grad()
    def sample(self, transfer_module, x_c, x_s, device):
        """models/RevResNet.py:241-263 (training-log helper; the fork's pdb trap is dropped)."""
        was_training = self.training
        self.eval()
        x_cs, x_c_cyc = [], []
        for i in range(x_c.size(0)):
            z_c = self(x_c[i].unsqueeze(0).to(device))
            z_s = self(x_s[i].unsqueeze(0).to(device))
            stylized = self(transfer_module.transfer(z_c, z_s), forward=False)
            z_cs = self(stylized)
            rec = self(transfer_module.transfer(z_cs, z_c), forward=False)
            x_cs.append(stylized.cpu())
            x_c_cyc.append(rec.cpu())
        if was_training:
            self.train()
        return x_c, x_s, torch.cat(x_cs), torch.cat(x_c_cyc)
