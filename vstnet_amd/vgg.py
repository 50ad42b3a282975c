"""Style loss on the device (csrc/vgg.hip; DESIGN.md section 6, "Style loss"): the reference's VGG-19 encoder up to relu4_1
(models/VGG.py), the mean / std records of its four taps, and the two numbers the reference trains on next to the affinity and
the temporal loss:

    loss_s = sum over relu1_1, relu2_1, relu3_1, relu4_1 of  mse(mean_a, mean_b) + mse(std_a, std_b)
    loss_c = mse(relu4_1(a), relu4_1(b))

``VGGEncoder`` holds the weights on one device, ``StyleLoss`` the records of one style and the buffers of one frame in flight;
``style_loss`` is the one-off call.  The kernel-level functions under them (one per kernel of csrc/vgg.hip) serve the tests and
tools.  Every call is queued on the current stream (or the one given) and never synchronises.  There is no CPU fallback: tensors
off the GPU raise ``ValueError``, a shape the kernels do not take raises ``VstError``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .resize import _ptr, _stream

LEVEL_CHANNELS = (64, 128, 256, 512)
RECORD_DOUBLES = _lib.VGG_RECORD_DOUBLES
RECORD_OFFSETS = (0, 128, 384, 896)
MIN_EDGE = 9                      # 9 -> 5 -> 3 -> 2: every level keeps an edge of at least 2 for the reflection
EPS = 1e-5                        # the reference's calc_mean_std


def level_sizes(h, w):
    """the four tap grids of an h x w frame: three ceil-mode 2 x 2 pools"""
    out = [(int(h), int(w))]
    for _ in range(3):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def workspace_bytes(h, w):
    """The bytes of device memory a features run on an h x w frame needs (vst_vgg_workspace_bytes; needs no GPU)."""
    n = C.c_size_t(0)
    _lib.check(_lib.lib().vst_vgg_workspace_bytes(int(h), int(w), C.byref(n)), "vst_vgg_workspace_bytes")
    return int(n.value)


def split_records(rec):
    """records [1920] -> [(mean [C], std [C])] of the four taps (views)"""
    return [(rec[o:o + c], rec[o + c:o + 2 * c]) for o, c in zip(RECORD_OFFSETS, LEVEL_CHANNELS)]


def indexed_device(device=None):
    """the torch.device of a GPU with its index spelt out ("cuda" is the current one), so that two of them compare"""
    import torch
    d = torch.device(device if device is not None else "cuda")
    if d.type != "cuda":
        raise ValueError("the style loss runs on the GPU (no CPU fallback)")
    return d if d.index is not None else torch.device("cuda", torch.cuda.current_device())


def _check_frame(x):
    """(tensor, True) for a uint8 [h,w,3] frame, (tensor, False) for a float32 [3,h,w] one; a leading batch of 1 is dropped"""
    import torch
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype not in (torch.float32, torch.uint8):
        raise ValueError("a frame must be a float32 [3,h,w] or uint8 [h,w,3] tensor on the GPU (no CPU fallback)")
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    u8 = x.dtype == torch.uint8
    if x.dim() != 3 or x.shape[2 if u8 else 0] != 3 or not x.is_contiguous():
        raise ValueError(f"expected a contiguous {'uint8 [h,w,3]' if u8 else 'float32 [3,h,w]'} frame, got {tuple(x.shape)}")
    return x, u8


def _frame_hw(x, u8):
    return (int(x.shape[0]), int(x.shape[1])) if u8 else (int(x.shape[1]), int(x.shape[2]))


def _f32_dev(t, name):
    import torch
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 tensor on the GPU (no CPU fallback)")
    return t


class VGGEncoder:
    """The encoder's weights on one device.  `weights`: a state dict with the reference checkpoint's keys ("0.weight" ...
    "29.bias"; later layers are ignored), or "synthetic" for synth.synthetic_vgg_state_dict()."""

    def __init__(self, weights="synthetic", device=None):
        import torch
        from .synth import synthetic_vgg_state_dict, vgg_state_dict_spec
        if isinstance(weights, str):
            if weights != "synthetic":
                raise ValueError('weights must be a state dict or "synthetic"')
            weights = synthetic_vgg_state_dict()
        self.device = indexed_device(device)
        self._plan = C.c_void_p(0)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            _lib.check(L.vst_vgg_create(C.byref(self._plan)), "vst_vgg_create")
            for key, shape in vgg_state_dict_spec(full=False):
                if key not in weights:
                    raise KeyError(f"the VGG state dict lacks {key}")
                t = weights[key].detach().to("cpu", torch.float32).contiguous()
                if tuple(t.shape) != tuple(shape):
                    raise ValueError(f"{key}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
                _lib.check(L.vst_vgg_load_tensor(self._plan, key.encode(), C.c_void_p(t.data_ptr()), t.numel()),
                           f"vst_vgg_load_tensor({key})")

    def __del__(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            try:
                _lib.lib().vst_vgg_destroy(plan)
            except Exception:
                pass

    def features(self, frame, records=None, relu4_1=None, ws=None, stream=None):
        """-> (records float64 [1920], relu4_1 or None).  relu4_1: True to allocate the float32 [h4*w4, 512] map, a tensor to
        fill, None to skip.  `records` and `ws` (uint8, at least workspace_bytes(h, w) bytes) are allocated when not given; `stream`
        needs `ws` (and tensors the caller keeps alive until that stream has run)."""
        import torch
        x, u8 = _check_frame(frame)
        h, w = _frame_hw(x, u8)
        if x.device != self.device:
            raise ValueError(f"the frame is on {x.device}, the encoder on {self.device}")
        if stream is not None and ws is None:
            raise ValueError("a call on a stream of its own brings its workspace: one allocated here would belong to torch's "
                             "current stream and be freed at return, while the launches on `stream` may still run")
        need = workspace_bytes(h, w)
        h4, w4 = level_sizes(h, w)[3]
        with torch.cuda.device(self.device):
            if records is None:
                records = torch.empty(RECORD_DOUBLES, dtype=torch.float64, device=self.device)
            elif records.dtype != torch.float64 or records.numel() != RECORD_DOUBLES or not records.is_contiguous() \
                    or records.device != self.device:
                raise ValueError(f"records must be a contiguous float64 [{RECORD_DOUBLES}] tensor on {self.device}")
            if relu4_1 is True:
                relu4_1 = torch.empty((h4 * w4, 512), dtype=torch.float32, device=self.device)
            elif relu4_1 is not None and (relu4_1.dtype != torch.float32 or relu4_1.numel() != h4 * w4 * 512
                                          or not relu4_1.is_contiguous() or relu4_1.device != self.device):
                raise ValueError(f"relu4_1 must be a contiguous float32 tensor of {h4 * w4} x 512 on {self.device}")
            if ws is None:
                ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.device != self.device:
                raise ValueError(f"ws must be a contiguous uint8 tensor of at least {need} bytes on {self.device}")
            name = "vst_vgg_features_u8" if u8 else "vst_vgg_features_f32"
            _lib.check(getattr(_lib.lib(), name)(self._plan, _ptr(x), h, w, _ptr(records), _ptr(relu4_1), _ptr(ws),
                                                 ws.numel(), _stream(stream)), name)
        return records, relu4_1


class StyleLoss:
    """loss_s of frames against ONE style, whose four records are computed once here (the style may have any size from 9 x 9);
    with a content frame also loss_c.  The workspace, the records and the two relu4_1 maps of a frame in flight belong to this
    object and are made at the first frame of a size, so one object serves one frame at a time (a pipeline keeps one per slot;
    ``clone()`` makes another that shares the encoder and the style's records)."""

    def __init__(self, encoder, style_frame=None, _style_records=None):
        import torch
        self.encoder = encoder
        self.device = encoder.device
        if _style_records is not None:
            self.style_records = _style_records
        else:
            self.style_records, _ = encoder.features(style_frame)
            with torch.cuda.device(self.device):
                torch.cuda.current_stream().synchronize()       # once, here: later calls read the records from any stream
        with torch.cuda.device(self.device):
            self.records = torch.empty(RECORD_DOUBLES, dtype=torch.float64, device=self.device)
            self.content_records = torch.empty(RECORD_DOUBLES, dtype=torch.float64, device=self.device)
            self.loss = torch.empty(2, dtype=torch.float64, device=self.device)
            self.mse_ws = torch.empty(_lib.VGG_MSE_WS_BYTES, dtype=torch.uint8, device=self.device)
        self.hw = None
        self.ws = self.map_x = self.map_c = None

    def clone(self):
        return StyleLoss(self.encoder, _style_records=self.style_records)

    def _buffers(self, h, w, content):
        import torch
        if self.hw != (h, w):
            h4, w4 = level_sizes(h, w)[3]
            with torch.cuda.device(self.device):
                self.ws = torch.empty(workspace_bytes(h, w), dtype=torch.uint8, device=self.device)
                self.map_x = torch.empty((h4 * w4, 512), dtype=torch.float32, device=self.device)
                self.map_c = None
            self.hw = (h, w)
        if content and self.map_c is None:
            with torch.cuda.device(self.device):
                self.map_c = torch.empty_like(self.map_x)

    def __call__(self, frame, content=None, out=None, stream=None):
        """-> device float64 (loss_s,) or, with `content`, (loss_s, loss_c): a view of this object's values or of `out`
        (float64, at least as many elements).  frame, content: uint8 [h,w,3] or float32 [3,h,w], of one size."""
        import torch
        x, u8 = _check_frame(frame)
        h, w = _frame_hw(x, u8)
        n = 1 if content is None else 2
        if content is not None:
            c, c_u8 = _check_frame(content)
            if _frame_hw(c, c_u8) != (h, w):
                raise ValueError(f"the content is {_frame_hw(c, c_u8)}, the frame {(h, w)}: loss_c needs one size")
        if out is None:
            out = self.loss
        elif not torch.is_tensor(out) or out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous float64 tensor of at least {n} elements on {self.device}")
        if h < MIN_EDGE or w < MIN_EDGE:
            _lib.check(-2, f"a style loss of a {h} x {w} frame (the smallest is {MIN_EDGE} x {MIN_EDGE})")
        self._buffers(h, w, content is not None)
        out = out.view(-1)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            self.encoder.features(x, self.records, self.map_x if content is not None else None, self.ws, stream)
            _lib.check(L.vst_vgg_style_loss(_ptr(self.records), _ptr(self.style_records), _ptr(out), _stream(stream)),
                       "vst_vgg_style_loss")
            if content is not None:
                self.encoder.features(c, self.content_records, self.map_c, self.ws, stream)
                _lib.check(L.vst_vgg_mse_f64(_ptr(self.map_x), _ptr(self.map_c), self.map_x.numel(), _ptr(out[1:]),
                                             _ptr(self.mse_ws), _stream(stream)), "vst_vgg_mse_f64")
        return out[:n]


def style_loss(encoder, frame, style_frame, content=None, out=None, stream=None):
    """One-off (loss_s[, loss_c]) of `frame` against `style_frame` (and `content`), a device float64 tensor."""
    res = StyleLoss(encoder, style_frame)(frame, content, out=out, stream=stream)
    return res if out is not None else res.clone()


# ------------------------------------------------------------------------------------------ kernel-level calls (tests, tools)
def input_map(frame, w9, b3, stream=None):
    """uint8 [h,w,3] or float32 [3,h,w] -> float32 [h*w, 4]: (x / 255 for bytes, then) the 1 x 1 conv, channel 3 zero"""
    import torch
    x, u8 = _check_frame(frame)
    h, w = _frame_hw(x, u8)
    w9, b3 = _f32_dev(w9, "w9"), _f32_dev(b3, "b3")
    if w9.numel() != 9 or b3.numel() != 3:
        raise ValueError("w9 holds 9 floats, b3 holds 3")
    out = torch.empty((h * w, 4), dtype=torch.float32, device=x.device)
    name = "vst_vgg_input_u8" if u8 else "vst_vgg_input_f32"
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.lib(), name)(_ptr(x), _ptr(w9), _ptr(b3), _ptr(out), h, w, _stream(stream)), name)
    return out


def conv3x3_relu(x, weight, bias, h, w, stream=None):
    """x float32 [h*w, Cin], weight float32 [Cout, 9*Cin] in K order (ky, kx, c), bias [Cout] -> float32 [h*w, Cout]"""
    import torch
    x, weight, bias = _f32_dev(x, "x"), _f32_dev(weight, "weight"), _f32_dev(bias, "bias")
    cin, cout = int(x.shape[1]), int(weight.shape[0])
    if x.shape[0] != h * w or weight.shape[1] != 9 * cin or bias.numel() != cout:
        raise ValueError(f"x {tuple(x.shape)}, weight {tuple(weight.shape)}, bias {tuple(bias.shape)} do not fit {h} x {w}")
    out = torch.empty((h * w, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vst_vgg_conv3x3_relu(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), int(h), int(w), cin, cout,
                                                   _stream(stream)), "vst_vgg_conv3x3_relu")
    return out


def maxpool2(x, h, w, stream=None):
    """x float32 [h*w, C] -> float32 [ceil(h/2)*ceil(w/2), C]"""
    import torch
    x = _f32_dev(x, "x")
    if x.shape[0] != h * w:
        raise ValueError(f"x {tuple(x.shape)} does not fit {h} x {w}")
    c = int(x.shape[1])
    out = torch.empty((((h + 1) // 2) * ((w + 1) // 2), c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vst_vgg_maxpool2(_ptr(x), _ptr(out), int(h), int(w), c, _stream(stream)), "vst_vgg_maxpool2")
    return out


def mean_std(x, eps=EPS, stream=None):
    """x float32 [n, C] -> float64 [2, C]: per channel the mean and sqrt(unbiased variance + eps), in fp64"""
    import torch
    x = _f32_dev(x, "x")
    n, c = int(x.shape[0]), int(x.shape[1])
    need = C.c_size_t(0)
    _lib.check(_lib.lib().vst_vgg_mean_std_workspace_bytes(n, c, C.byref(need)), "vst_vgg_mean_std_workspace_bytes")
    out = torch.empty((2, c), dtype=torch.float64, device=x.device)
    ws = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vst_vgg_mean_std(_ptr(x), n, c, float(eps), _ptr(out), _ptr(ws), ws.numel(), _stream(stream)),
                   "vst_vgg_mean_std")
    return out


def mse_f64(a, b, stream=None):
    """mean((a - b)^2) of two equal-shaped float32 tensors in fp64 -> float64 [1]"""
    import torch
    a, b = _f32_dev(a, "a"), _f32_dev(b, "b")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("a and b must have one shape and one device")
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    ws = torch.empty(_lib.VGG_MSE_WS_BYTES, dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().vst_vgg_mse_f64(_ptr(a), _ptr(b), a.numel(), _ptr(out), _ptr(ws), _stream(stream)),
                   "vst_vgg_mse_f64")
    return out


def style_loss_of_records(rec_a, rec_b, stream=None):
    """two float64 [1920] record sets -> float64 [1]"""
    import torch
    for r in (rec_a, rec_b):
        if not torch.is_tensor(r) or not r.is_cuda or r.dtype != torch.float64 or r.numel() != RECORD_DOUBLES \
                or not r.is_contiguous():
            raise ValueError(f"records are contiguous float64 [{RECORD_DOUBLES}] tensors on the GPU")
    out = torch.empty(1, dtype=torch.float64, device=rec_a.device)
    with torch.cuda.device(rec_a.device):
        _lib.check(_lib.lib().vst_vgg_style_loss(_ptr(rec_a), _ptr(rec_b), _ptr(out), _stream(stream)), "vst_vgg_style_loss")
    return out
