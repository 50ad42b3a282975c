"""SegFormer (MiT-B1..B5 + MLP decode head) on the device (csrc/segformer.hip): the segmenter behind ``--auto_seg``.

The reference's ``SegmentModel`` (project/image_style/segment.py:471-532) fixes the arithmetic.  This module turns its state
dict into the tensors the library wants - conv weights in the patch gather's K order, the decode head folded in fp64 - and
wraps a ``vst_seg`` plan.  There is no torch implementation behind it: a missing library or kernel is an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .synth import SEG_CLASSES, SEG_DEPTHS, SEG_EMBED_DIMS, SEG_SR_RATIOS, segformer_state_dict_spec

IGNORED_PREFIXES = ("decode_head.conv_seg.", "label_mapping")
BN_EPS = 1e-5
MAX_PIXELS = 1 << 24          # csrc/segformer.hip SEG_MAX_PIXELS: the (working) frame the network runs on; no tiled segmentation
MAX_LABEL_PIXELS = 1 << 30    # vstnet.h VST_SEG_MAX_LABEL_PIXELS: the label map a working frame is sampled to
MIN_WORK_SIZE = 32
MAX_WINDOW = _lib.SEG_MIX_MAX  # frames vst_seg_mix_logits mixes (--seg_window)


def window_weights(n_available: int, decay: float = 1.0):
    """fp32 weights by age (index 0 = the current frame) of a temporal logit window over the ``n_available`` frames that exist:
    proportional to decay**k, normalised in double to sum 1.  At the start of a clip fewer than --seg_window frames exist; the
    window is then those frames, renormalised."""
    n = int(n_available)
    if not 1 <= n <= MAX_WINDOW:
        raise ValueError(f"a window holds 1..{MAX_WINDOW} frames, got {n_available}")
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"decay must be in (0, 1] (--seg_decay), got {decay}")
    w = np.power(np.float64(decay), np.arange(n, dtype=np.float64))
    return (w / w.sum()).astype(np.float32)


def _f64(t):
    return (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(np.float64)


def fold_decode_head(sd, embedding_dim: int = 768):
    """The decode head with ``linear_fuse`` pushed through the bilinear upsampling, in fp64.

    ``linear_fuse.conv`` is a bias-free 1x1 conv over cat[up(c4'), up(c3'), up(c2'), c1'] with c_i' = W_ci x_i + b_ci.  A 1x1
    conv commutes with bilinear upsampling and the upsampling weights sum to one, so
        fuse = sum_i up(s * W_fuse[:, slice_i] W_ci x_i)  +  s * (sum_i W_fuse[:, slice_i] b_ci - mean) + beta
    with s = gamma / sqrt(var + eps) of the eval-mode BatchNorm.  Returns {"fold_c{i}.weight": [E, C_i], "fold.bias": [E]}."""
    e = embedding_dim
    wf = _f64(sd["decode_head.linear_fuse.conv.weight"]).reshape(e, 4 * e)
    s = _f64(sd["decode_head.linear_fuse.bn.weight"]) / np.sqrt(_f64(sd["decode_head.linear_fuse.bn.running_var"]) + BN_EPS)
    bias = np.zeros(e)
    out = {}
    for slot, i in enumerate((4, 3, 2, 1)):          # the order of torch.cat([_c4, _c3, _c2, _c1])
        w_slice = wf[:, slot * e:(slot + 1) * e]
        out[f"fold_c{i}.weight"] = s[:, None] * (w_slice @ _f64(sd[f"decode_head.linear_c{i}.proj.weight"]))
        bias += w_slice @ _f64(sd[f"decode_head.linear_c{i}.proj.bias"])
    out["fold.bias"] = s * (bias - _f64(sd["decode_head.linear_fuse.bn.running_mean"])) + _f64(sd["decode_head.linear_fuse.bn.bias"])
    return out


def check_state_dict(sd, depths, embedding_dim):
    """Exactly the reference's keys and shapes; the ignored entries may be present or absent."""
    if "state_dict" in sd and not hasattr(sd["state_dict"], "shape"):
        sd = sd["state_dict"]
    for key, shp in segformer_state_dict_spec(depths, embedding_dim):
        if key.startswith(IGNORED_PREFIXES) or key.endswith("num_batches_tracked"):
            continue
        if key not in sd:
            raise KeyError(f"SegFormer state dict: missing key {key}")
        if tuple(sd[key].shape) != tuple(shp):
            raise ValueError(f"SegFormer state dict: {key} has shape {tuple(sd[key].shape)}, expected {tuple(shp)}")
    known = {k for k, _ in segformer_state_dict_spec(depths, embedding_dim)}
    extra = [k for k in sd if k not in known and not k.startswith(IGNORED_PREFIXES)]
    if extra:
        raise KeyError(f"SegFormer state dict: unexpected key {extra[0]}")
    return sd


def library_tensors(sd, depths, embedding_dim: int = 768):
    """name -> fp32 C-contiguous numpy array in the layout include/vstnet.h documents for vst_seg_load_tensor."""
    out = {}
    head = fold_decode_head(sd, embedding_dim)
    for key, shp in segformer_state_dict_spec(depths, embedding_dim):
        if not key.startswith("backbone."):
            continue
        a = _f64(sd[key])
        if key.endswith("dwconv.dwconv.weight"):
            a = a.reshape(shp[0], 9).T                        # [9][C]
        elif a.ndim == 4:
            a = a.transpose(0, 2, 3, 1)                       # [out][ky][kx][in]
        out[key] = a
    for k, v in head.items():
        out["decode_head." + k] = v
    out["decode_head.linear_pred.weight"] = _f64(sd["decode_head.linear_pred.weight"]).reshape(SEG_CLASSES, embedding_dim)
    out["decode_head.linear_pred.bias"] = _f64(sd["decode_head.linear_pred.bias"])
    return {k: np.ascontiguousarray(v.astype(np.float32)).reshape(-1) for k, v in out.items()}


def stage_grids(height: int, width: int):
    """[(h_i, w_i)] of the four stages for an H x W frame (vst_seg_shape)."""
    hw = (C.c_int * 8)()
    _lib.check(_lib.lib().vst_seg_shape(int(height), int(width), hw), "vst_seg_shape")
    return [(hw[2 * i], hw[2 * i + 1]) for i in range(4)]


class SegFormer:
    """``SegmentModel`` on one GPU.  ``segment_u8`` is stream-ordered on torch's current stream; every stream gets its own
    workspace inside the plan, so frames may be in flight on several streams at once."""

    def __init__(self, variant: str = "b4", depths=None, embedding_dim: int = 768, device=None):
        import torch
        if depths is None:
            if variant not in SEG_DEPTHS:
                raise ValueError(f"variant must be one of {sorted(SEG_DEPTHS)} (MiT-B0 is not supported)")
            depths = SEG_DEPTHS[variant]
        self.depths = tuple(int(d) for d in depths)
        self.embedding_dim = int(embedding_dim)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SegFormer runs on the GPU only (no CPU fallback)")
        if self.device.index is None:           # "cuda" means the current device; tensors always carry an index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._plan = C.c_void_p(0)
        self.loaded = False
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().vst_seg_create((C.c_int * 4)(*self.depths), self.embedding_dim, C.byref(self._plan)),
                       "vst_seg_create")

    def __del__(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            try:
                _lib.lib().vst_seg_destroy(plan)
            except Exception:        # interpreter shutdown
                pass

    def tensor_table(self):
        """[(name, count)] the plan expects."""
        L = _lib.lib()
        out = []
        for i in range(L.vst_seg_tensor_count(self._plan)):
            name, count = C.c_char_p(), C.c_size_t()
            _lib.check(L.vst_seg_tensor_info(self._plan, i, C.byref(name), C.byref(count)), "vst_seg_tensor_info")
            out.append((name.value.decode(), count.value))
        return out

    def load_state_dict(self, sd):
        import torch
        sd = check_state_dict(sd, self.depths, self.embedding_dim)
        tensors = library_tensors(sd, self.depths, self.embedding_dim)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for name, count in self.tensor_table():
                a = tensors[name]
                if a.size != count:
                    raise ValueError(f"{name}: {a.size} values, the plan expects {count}")
                _lib.check(L.vst_seg_load_tensor(self._plan, name.encode(), a.ctypes.data_as(C.c_void_p), a.size),
                           f"vst_seg_load_tensor({name})")
        self.loaded = True
        return self

    @staticmethod
    def work_hw(height: int, width: int, work_size):
        """The size (h, w) an H x W frame is segmented at for ``work_size`` = the long edge of the working frame: (H, W) itself
        when that is no shrink (or ``work_size`` is None), else both edges scaled by work_size / max(H, W), rounded half up and
        kept >= 32."""
        h, w = int(height), int(width)
        if work_size is None:
            return h, w
        if int(work_size) != work_size or work_size < MIN_WORK_SIZE:
            raise ValueError(f"work_size must be an integer >= {MIN_WORK_SIZE} (--seg_size), got {work_size}")
        f = int(work_size) / max(h, w)
        if f >= 1:
            return h, w
        return max(MIN_WORK_SIZE, int(h * f + 0.5)), max(MIN_WORK_SIZE, int(w * f + 0.5))

    def _frame(self, frame_u8, limit=MAX_PIXELS):
        import torch
        if not torch.is_tensor(frame_u8) or frame_u8.dtype != torch.uint8 or frame_u8.device != self.device:
            raise ValueError(f"frame_u8 must be a uint8 tensor on {self.device} (no CPU fallback)")
        if frame_u8.dim() != 3 or 3 not in (frame_u8.shape[0], frame_u8.shape[2]):
            raise ValueError(f"expected [H,W,3] or [3,H,W], got {tuple(frame_u8.shape)}")
        if not self.loaded:
            raise _lib.VstError("SegFormer: load_state_dict has not been called")
        chw = 0 if frame_u8.shape[2] == 3 else 1
        h, w = (frame_u8.shape[1], frame_u8.shape[2]) if chw else (frame_u8.shape[0], frame_u8.shape[1])
        if limit is not None and h * w > limit:
            raise ValueError(f"--auto_seg segments whole frames of at most {limit} pixels; {h}x{w} is larger and there is no "
                             "tiled segmentation (--seg_size segments a downscaled copy)")
        return frame_u8.contiguous(), chw, int(h), int(w)

    def _labels(self, out, h, w):
        import torch
        if out is None:
            return torch.empty((h, w), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (h, w) or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous uint8 [H,W] tensor on the segmenter's device")
        return out

    def _run_scaled(self, work, chw, hw, ww, h, w, out):
        import torch
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().vst_seg_run_scaled_u8(self._plan, C.c_void_p(work.data_ptr()), chw, hw, ww, h, w,
                                                        C.c_void_p(out.data_ptr()), st), "vst_seg_run_scaled_u8")
        return out

    def segment_u8(self, frame_u8, out=None, work_size=None, work=None):
        """uint8 [H,W,3] or [3,H,W] on the device -> uint8 [H,W] labels on the device (into ``out`` when given).

        work_size: segment a PIL-exact bicubic downscale of the frame (``work_hw``; vstnet_amd.resize.resize_u8, queued on the
        current stream) and sample the quarter-resolution logits at the frame's own size in one bilinear step.  ``work`` is the
        caller's uint8 buffer of at least h_w * w_w * 3 bytes for that copy (allocated when None).  A frame that ``work_size``
        does not shrink takes the plain route, with the same labels as without it."""
        import torch
        f, chw, h, w = self._frame(frame_u8, limit=MAX_PIXELS if work_size is None else MAX_LABEL_PIXELS)
        hw, ww = self.work_hw(h, w, work_size)
        if (hw, ww) == (h, w):
            if h * w > MAX_PIXELS:          # (a work_size that does not shrink the frame: the whole-frame limit holds)
                self._frame(frame_u8)
            out = self._labels(out, h, w)
            with torch.cuda.device(self.device):
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                _lib.check(_lib.lib().vst_seg_run_u8(self._plan, C.c_void_p(f.data_ptr()), chw, h, w, C.c_void_p(out.data_ptr()), st),
                           "vst_seg_run_u8")
            return out
        from .resize import MAX_SHRINK, resize_u8
        if h > MAX_SHRINK * hw or w > MAX_SHRINK * ww:
            raise ValueError(f"--seg_size {work_size} shrinks a {w}x{h} frame to {ww}x{hw}: more than the device resize's "
                             f"{MAX_SHRINK}x per axis (VST_RESIZE_MAX_SHRINK); raise --seg_size")
        out = self._labels(out, h, w)
        if chw:
            f = f.permute(1, 2, 0).contiguous()
        if work is not None:
            if work.dtype != f.dtype or work.device != self.device or not work.is_contiguous() or work.numel() < hw * ww * 3:
                raise ValueError(f"work must be a contiguous uint8 tensor of at least {hw * ww * 3} bytes on {self.device}")
            work = work.view(-1)[:hw * ww * 3].view(hw, ww, 3)
        work = resize_u8(f, (ww, hw), out=work)
        return self._run_scaled(work, 0, hw, ww, h, w, out)

    def segment_work_u8(self, work_u8, out_hw, out=None):
        """A frame that is ALREADY at its working size (e.g. resized by PIL on the host and uploaded) -> uint8 labels at
        ``out_hw`` = (H, W), H * W <= MAX_LABEL_PIXELS: what ``segment_u8(frame, work_size=...)`` does after its resize."""
        f, chw, hw, ww = self._frame(work_u8)
        h, w = int(out_hw[0]), int(out_hw[1])
        return self._run_scaled(f, chw, hw, ww, h, w, self._labels(out, h, w))

    def logit_grid(self, height: int, width: int):
        """(Hq, Wq) of the logits of an H x W (working) frame."""
        return stage_grids(height, width)[0]

    def logits_into(self, frame_u8, out):
        """The quarter-resolution logits of a frame (or of a frame already at its working size), token-major, into the caller's
        contiguous fp32 [Hq*Wq, 150] buffer: stream-ordered on the current stream, nothing else is written."""
        import torch
        f, chw, h, w = self._frame(frame_u8)
        hq, wq = self.logit_grid(h, w)
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (hq * wq, SEG_CLASSES)
                or not out.is_contiguous() or out.device != self.device):
            raise ValueError(f"out must be a contiguous float32 [{hq * wq},{SEG_CLASSES}] tensor on {self.device}")
        null = C.c_void_p(0)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().vst_seg_logits(self._plan, C.c_void_p(f.data_ptr()), chw, h, w, C.c_void_p(out.data_ptr()),
                                                 null, null, null, null, st), "vst_seg_logits")
        return out

    def mix_logits(self, logit_list, weights, out):
        """out = sum_k weights[k] * logit_list[k] (vst_seg_mix_logits: index 0 = the current frame, every product and sum
        rounded to fp32 in that order), on the current stream.  The tensors are contiguous fp32 of one shape on this device;
        ``out`` is none of them."""
        import torch
        n = len(logit_list)
        if n != len(weights):
            raise ValueError(f"{n} logit tensors and {len(weights)} weights")
        for t in list(logit_list) + [out]:
            if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device
                    or t.shape != out.shape):
                raise ValueError(f"mix_logits takes contiguous float32 tensors of one shape on {self.device}")
        ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in logit_list])
        ws = (C.c_float * max(n, 1))(*[float(w) for w in weights])
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().vst_seg_mix_logits(ptrs, ws, n, out.numel(), C.c_void_p(out.data_ptr()), st),
                       "vst_seg_mix_logits")
        return out

    def labels_from_logits(self, logits, grid_hw, out_hw, out=None):
        """Token-major logits [Hq*Wq, 150] of the grid ``grid_hw`` -> uint8 labels at ``out_hw``: the sampling + argmax step of a
        run (vst_seg_labels_from_logits, the run's own choice of sampler), on the current stream."""
        import torch
        hq, wq = int(grid_hw[0]), int(grid_hw[1])
        h, w = int(out_hw[0]), int(out_hw[1])
        if (not torch.is_tensor(logits) or logits.dtype != torch.float32 or logits.numel() != hq * wq * SEG_CLASSES
                or not logits.is_contiguous() or logits.device != self.device):
            raise ValueError(f"logits must be contiguous float32 [{hq * wq},{SEG_CLASSES}] on {self.device}")
        out = self._labels(out, h, w)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().vst_seg_labels_from_logits(C.c_void_p(logits.data_ptr()), hq, wq, h, w, -1,
                                                             C.c_void_p(out.data_ptr()), st), "vst_seg_labels_from_logits")
        return out

    def logits(self, frame_u8):
        """(quarter-resolution logits [150, Hq, Wq], [x1..x4] as [C_i, h_i, w_i]) - for tests."""
        import torch
        f, chw, h, w = self._frame(frame_u8)
        grids = stage_grids(h, w)
        lg = torch.empty((grids[0][0] * grids[0][1], SEG_CLASSES), dtype=torch.float32, device=self.device)
        xs = [torch.empty((gh * gw, c), dtype=torch.float32, device=self.device) for (gh, gw), c in zip(grids, SEG_EMBED_DIMS)]
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().vst_seg_logits(self._plan, C.c_void_p(f.data_ptr()), chw, h, w, C.c_void_p(lg.data_ptr()),
                                                 *[C.c_void_p(x.data_ptr()) for x in xs], st), "vst_seg_logits")
        planar = lambda t, g: t.reshape(g[0], g[1], -1).permute(2, 0, 1)      # noqa: E731
        return planar(lg, grids[0]), [planar(x, g) for x, g in zip(xs, grids)]


from . import segformer_ops as ops  # noqa: E402,F401  (vstnet_amd.segformer.ops: the kernels one by one, for tests and tools)
