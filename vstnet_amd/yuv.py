"""Raw video edge ("Raw video edge" and "High-bit-depth edge"), both depths:

  YuvSpec      8-bit Y'CbCr planes <-> uint8 HWC RGB frames (vst_yuv_to_rgb_u8, vst_rgb_to_yuv_u8): a YUV4MPEG2 frame goes up
               and comes back as the 1.5 bytes per pixel it is on disk.
  DeepYuvSpec  9..16-bit planes <-> fp32 RGB planes on a 0..1 scale (vst_yuv16_to_rgb_f32, vst_rgb_f32_to_yuv16): a frame of
               headerless raw YUV (yuv420p10le, yuv422p10le, ...; vstnet_amd/rawyuv.py) enters the encoder and leaves the decoder
               as float planes, so nothing between the file and the network passes through 256 levels.

Pointwise HIP kernels (csrc/yuv.hip) on device tensors, on the current stream, one launch each way.  There is no CPU path for
those.  DeepImgResize / yuv16_img_resize_f32: a deep frame of any size to the stylised size - img_resize restated in float, fused
with the conversion (vst_yuv16_img_resize_f32; the numpy statement is resize.img_resize_float of yuv16_to_rgb_float).  The *_float / *_host functions state the same arithmetic in numpy float64 (include/vstnet.h has it in words): the tests'
reference, and what `video_transfer.py --stub_stylise` rehearses with."""
from __future__ import annotations

import numpy as np

LAYOUTS = {"444": 0, "420jpeg": 1, "420mpeg2": 2, "422": 3}       # vstnet.h VST_YUV_444, _420_CENTRE, _420_LEFT, _422
MATRICES = {"bt601": (0, 0.299, 0.114), "bt709": (1, 0.2126, 0.0722)}            # (VST_YUV_BT*, Kr, Kb)
RANGES = {"limited": 0, "full": 1}
DEPTHS = tuple(range(9, 17))
TIE_EPS = 2.0 ** -10     # the 8-bit kernels' fp32 arithmetic errs by under 6e-5 on these magnitudes: a byte may differ only this close to a tie
DEEP_TIE_EPS = 2.0 ** -20        # the deep kernels' fp64 arithmetic errs by under 2^-32 of a code: a code may differ only this close


class _Spec:
    """How a frame's planes are laid out and what their codes mean.  A subclass names its layouts and its depths."""
    _LAYOUTS, _DEPTHS, _DEPTHS_TEXT = (), (), ""

    def __init__(self, layout, matrix, range, depth):
        if layout not in self._LAYOUTS or matrix not in MATRICES or range not in RANGES or depth not in self._DEPTHS:
            got = (layout, matrix, range) + ((depth,) if self._DEPTHS_TEXT else ())
            raise ValueError(f"{type(self).__name__}: layout in {sorted(self._LAYOUTS)}, matrix in {sorted(MATRICES)}, range in "
                             f"{sorted(RANGES)}{self._DEPTHS_TEXT}; got {', '.join(repr(g) for g in got)}")
        self.layout, self.matrix, self.range, self.depth = layout, matrix, range, int(depth)

    def __eq__(self, other):
        return type(other) is type(self) and self.codes == other.codes

    def __hash__(self):
        return hash((type(self).__name__,) + self.codes)

    @property
    def max_code(self):
        return (1 << self.depth) - 1

    @property
    def sample_bytes(self):
        return 1 if self.depth == 8 else 2

    @property
    def scales(self):
        """(Y offset, Y scale, chroma offset, chroma scale) in codes"""
        s = float(1 << (self.depth - 8))
        coff = float(1 << (self.depth - 1))
        if self.range == "limited":
            return 16.0 * s, 219.0 * s, coff, 224.0 * s
        return 0.0, float(self.max_code), coff, float(self.max_code)

    def plane_shapes(self, H, W):
        """((H, W), chroma, chroma) in samples: chroma planes are H x ceil(W/2) at 4:2:2, ceil(H/2) x ceil(W/2) at 4:2:0"""
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"a frame is at least 1x1, got {W}x{H}")
        c = (H, W) if self.layout == "444" else (H, (W + 1) // 2) if self.layout == "422" else ((H + 1) // 2, (W + 1) // 2)
        return (H, W), c, c

    def frame_bytes(self, H, W):
        y, c, _ = self.plane_shapes(H, W)
        return self.sample_bytes * (y[0] * y[1] + 2 * c[0] * c[1])

    def split(self, flat, H, W):
        """The (y, u, v) views of one flat Y|U|V buffer (numpy array or torch tensor).  Two bytes per sample: the buffer is uint8
        (a torch buffer must start on a 2-byte address) and the views are 16-bit - numpy '<u2' arrays, torch int16 tensors: the
        same 16 bits, there to be pointed at and copied, not computed with."""
        ys, cs, _ = self.plane_shapes(H, W)
        ny, nc = ys[0] * ys[1], cs[0] * cs[1]
        deep = self.sample_bytes == 2
        if flat.ndim != 1 or flat.shape[0] != self.frame_bytes(H, W) or (deep and not str(flat.dtype).endswith("uint8")):
            raise ValueError(f"a {W}x{H} {self.layout} frame of {self.depth} bits is one flat uint8 buffer of {self.frame_bytes(H, W)} "
                             f"bytes, got {flat.dtype} {tuple(flat.shape)}" if deep else
                             f"a {W}x{H} {self.layout} frame is one flat buffer of {ny + 2 * nc} bytes, got shape {tuple(flat.shape)}")
        if deep and isinstance(flat, np.ndarray):
            flat = flat.view("<u2")
        elif deep:
            import torch
            flat = flat.view(torch.int16)
        return flat[:ny].reshape(ys), flat[ny:ny + nc].reshape(cs), flat[ny + nc:].reshape(cs)


class YuvSpec(_Spec):
    """8-bit planes: layout '444' | '420jpeg' (chroma centred in its 2 x 2 luma block; y4m C420jpeg and C420) | '420mpeg2'
    (horizontally on the even luma columns; C420mpeg2), matrix 'bt601' | 'bt709', range 'limited' | 'full'."""
    _LAYOUTS, _DEPTHS = ("444", "420jpeg", "420mpeg2"), (8,)

    def __init__(self, layout="420jpeg", matrix="bt601", range="limited"):
        super().__init__(layout, matrix, range, 8)

    def __repr__(self):
        return f"YuvSpec({self.layout!r}, {self.matrix!r}, {self.range!r})"

    @property
    def codes(self):
        """(layout, matrix, range) as the library's enums"""
        return LAYOUTS[self.layout], MATRICES[self.matrix][0], RANGES[self.range]


class DeepYuvSpec(_Spec):
    """High-bit-depth planes: layout '444' | '422' (chroma on the even luma columns, every row) | '420jpeg' | '420mpeg2' (as
    YuvSpec), matrix 'bt601' | 'bt709', range 'limited' | 'full', depth 9..16 bits in little-endian 16-bit samples."""
    _LAYOUTS, _DEPTHS, _DEPTHS_TEXT = tuple(LAYOUTS), DEPTHS, ", depth in 9..16"

    def __init__(self, layout="420mpeg2", matrix="bt709", range="limited", depth=10):
        super().__init__(layout, matrix, range, depth)

    def __repr__(self):
        return f"DeepYuvSpec({self.layout!r}, {self.matrix!r}, {self.range!r}, {self.depth})"

    @property
    def codes(self):
        """(layout, matrix, range, depth) as the library's enums and the depth"""
        return LAYOUTS[self.layout], MATRICES[self.matrix][0], RANGES[self.range], self.depth


def _want(spec, cls, what):
    if not isinstance(spec, cls):
        raise ValueError(f"{what} takes a {cls.__name__}")


# ---------------------------------------------------------------------------------------------------------------------------
# the arithmetic in float64
# ---------------------------------------------------------------------------------------------------------------------------
def round_bytes(v):
    """clamp(floor(v + 0.5), 0, 255) as uint8"""
    return np.clip(np.floor(np.asarray(v, np.float64) + 0.5), 0, 255).astype(np.uint8)


def round_codes(v, spec):
    """clamp(floor(v + 0.5), 0, 2^depth - 1) as uint16"""
    return np.clip(np.floor(np.asarray(v, np.float64) + 0.5), 0, spec.max_code).astype(np.uint16)


def near_tie(v, eps=TIE_EPS):
    """where v lies within eps of a rounding tie (x.5): the values the kernels may round the other way"""
    v = np.asarray(v, np.float64)
    return np.abs((v - np.floor(v)) - 0.5) < eps


def _taps(n_luma, n_chroma, centred):
    """bilinear taps of the luma positions 0..n_luma-1 in a chroma axis: (index a, index b, weight of b), indices clamped"""
    x = np.arange(n_luma, dtype=np.float64)
    f = (x - 0.5) / 2 if centred else x / 2
    i0 = np.floor(f)
    w = f - i0
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, n_chroma - 1), np.clip(i0 + 1, 0, n_chroma - 1), w


def upsample_chroma(plane, H, W, layout):
    """a subsampled plane sampled bilinearly at every luma position: float64 [H, W].  Columns are centred ('420jpeg') or
    left-sited; rows are centred, or at '422' the plane's own"""
    p = np.asarray(plane, np.float64)
    ja, jb, wx = _taps(W, p.shape[1], layout == "420jpeg")
    if layout == "422":
        return (1 - wx) * p[:, ja] + wx * p[:, jb]
    ia, ib, wy = _taps(H, p.shape[0], True)
    top = (1 - wx) * p[ia][:, ja] + wx * p[ia][:, jb]
    bot = (1 - wx) * p[ib][:, ja] + wx * p[ib][:, jb]
    return (1 - wy)[:, None] * top + wy[:, None] * bot


def downsample_chroma(c, layout):
    """float [H, W] chroma -> float [ceil(H/2), ceil(W/2)] ([H, ceil(W/2)] at '422'): columns averaged in pairs ('420jpeg') or
    with [1/4, 1/2, 1/4] around the even column; then rows averaged in pairs, except at '422'; a missing neighbour is the edge
    sample again"""
    c = np.asarray(c, np.float64)
    H, W = c.shape
    j = 2 * np.arange((W + 1) // 2)
    if layout == "420jpeg":
        h = 0.5 * (c[:, j] + c[:, np.minimum(j + 1, W - 1)])
    else:
        h = 0.25 * c[:, np.maximum(j - 1, 0)] + 0.5 * c[:, j] + 0.25 * c[:, np.minimum(j + 1, W - 1)]
    if layout == "422":
        return h
    i = 2 * np.arange((H + 1) // 2)
    return 0.5 * (h[i] + h[np.minimum(i + 1, H - 1)])


def _planes(planes_or_flat, H, W, spec):
    if isinstance(planes_or_flat, (tuple, list)):
        y, u, v = planes_or_flat
        for name, p, s in zip("yuv", (y, u, v), spec.plane_shapes(H, W)):
            if tuple(p.shape) != s:
                raise ValueError(f"plane {name} of a {W}x{H} {spec.layout} frame is {s}, got {tuple(p.shape)}")
        return y, u, v
    return spec.split(planes_or_flat, H, W)


def _codes_at_luma(planes_or_flat, H, W, spec):
    """float64 Y, U, V of every pixel: a deep code first limited to 2^depth - 1, chroma sampled at the luma positions"""
    def codes(p):           # (an int16 plane is a torch view of the same 16 bits)
        p = np.asarray(p)
        if spec.depth == 8:
            return p.astype(np.float64)
        return np.minimum((p.view(np.uint16) if p.dtype == np.int16 else p).astype(np.float64), spec.max_code)
    y, u, v = (codes(p) for p in _planes(planes_or_flat, H, W, spec))
    if spec.layout != "444":
        u, v = upsample_chroma(u, H, W, spec.layout), upsample_chroma(v, H, W, spec.layout)
    return y, u, v


def _matrix_to_rgb(yy, pb, pr, spec):
    _, kr, kb = MATRICES[spec.matrix]
    kg = 1.0 - kr - kb
    r = yy + 2 * (1 - kr) * pr
    b = yy + 2 * (1 - kb) * pb
    g = yy - (2 * (1 - kr) * kr / kg) * pr - (2 * (1 - kb) * kb / kg) * pb
    return np.stack([r, g, b], axis=-1)


def _matrix_to_ycc(rgb, spec, prepare):
    """Y and the (downsampled) Cb, Cr of an [H, W, 3] frame whose channels `prepare` makes float64"""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected an [H, W, 3] frame, got {tuple(rgb.shape)}")
    _, kr, kb = MATRICES[spec.matrix]
    kg = 1.0 - kr - kb
    r, g, b = (prepare(rgb[..., k].astype(np.float64)) for k in range(3))
    y = kr * r + kg * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if spec.layout != "444":
        cb, cr = downsample_chroma(cb, spec.layout), downsample_chroma(cr, spec.layout)
    return y, cb, cr


def yuv_to_rgb_float(planes_or_flat, H, W, spec):
    """the unrounded R, G, B of every pixel on the 0..255 scale: float64 [H, W, 3]"""
    y, u, v = _codes_at_luma(planes_or_flat, H, W, spec)
    yoff, ys, coff, cs = spec.scales
    return _matrix_to_rgb((y - yoff) * 255.0 / ys, (u - coff) * 255.0 / cs, (v - coff) * 255.0 / cs, spec)


def yuv_to_rgb_host(planes_or_flat, H, W, spec):
    """uint8 [H, W, 3]"""
    return round_bytes(yuv_to_rgb_float(planes_or_flat, H, W, spec))


def rgb_to_yuv_float(rgb, spec):
    """rgb: [H, W, 3] on the 0..255 scale.  The unrounded codes of the three planes, one flat float64 array Y|U|V"""
    y, cb, cr = _matrix_to_ycc(rgb, spec, lambda c: c)
    yoff, ys, coff, cs = spec.scales
    return np.concatenate([(yoff + y * ys / 255.0).reshape(-1), (coff + cb * cs / 255.0).reshape(-1),
                           (coff + cr * cs / 255.0).reshape(-1)])


def rgb_to_yuv_host(rgb, spec):
    """flat uint8 Y|U|V (spec.split gives the planes)"""
    return round_bytes(rgb_to_yuv_float(rgb, spec))


def yuv16_to_rgb_float(planes_or_flat, H, W, spec):
    """the unrounded R, G, B of every pixel on the 0..1 scale, clamped to [0, 1]: float64 [H, W, 3]"""
    y, u, v = _codes_at_luma(planes_or_flat, H, W, spec)
    yoff, ys, coff, cs = spec.scales
    return np.clip(_matrix_to_rgb((y - yoff) / ys, (u - coff) / cs, (v - coff) / cs, spec), 0.0, 1.0)


def yuv16_to_rgb_host(planes_or_flat, H, W, spec):
    """(float32 [H, W, 3] on the 0..1 scale, uint8 [H, W, 3] = floor(255 v + 0.5)): what the kernel's two outputs hold"""
    v = yuv16_to_rgb_float(planes_or_flat, H, W, spec)
    return v.astype(np.float32), np.floor(255.0 * v + 0.5).astype(np.uint8)


def rgb_to_yuv16_float(rgb, spec):
    """rgb: [H, W, 3] on the 0..1 scale (clamped here).  The unrounded codes of the three planes, one flat float64 array Y|U|V"""
    y, cb, cr = _matrix_to_ycc(rgb, spec, lambda c: np.clip(c, 0.0, 1.0))
    yoff, ys, coff, cs = spec.scales
    return np.concatenate([(yoff + y * ys).reshape(-1), (coff + cb * cs).reshape(-1), (coff + cr * cs).reshape(-1)])


def rgb_to_yuv16_host(rgb, spec):
    """flat uint8 Y|U|V, two bytes per sample, little-endian (spec.split gives the planes)"""
    return round_codes(rgb_to_yuv16_float(rgb, spec), spec).astype("<u2").view(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# the device calls
# ---------------------------------------------------------------------------------------------------------------------------
def _device_planes(planes_or_flat, H, W, spec, what):
    """the planes as device tensors: uint8 for a YuvSpec, any 16-bit integer type on a 2-byte address for a DeepYuvSpec"""
    import torch
    planes = _planes(planes_or_flat, H, W, spec)
    for p in planes:
        ok = torch.is_tensor(p) and p.is_cuda and p.is_contiguous()
        if spec.depth == 8:
            if not (ok and p.dtype == torch.uint8):
                raise ValueError(f"{what}: the planes are contiguous uint8 tensors on the GPU (no CPU fallback)")
        elif not (ok and p.element_size() == 2 and not p.is_floating_point() and p.data_ptr() % 2 == 0):
            raise ValueError(f"{what}: the planes are contiguous 16-bit integer tensors on the GPU, or one flat uint8 tensor on a "
                             "2-byte address (no CPU fallback)")
    return planes


def _frame_hw(x, what, planar=False):
    """(H, W) of a uint8 [H,W,3] frame, or of float32 [3,H,W] planes if `planar`; a leading axis of 1 is allowed"""
    import torch
    dtype, c, shape = (torch.float32, -3, "float32 [1,3,H,W] (or [3,H,W])") if planar else (torch.uint8, -1, "uint8 [H,W,3] (or [1,H,W,3])")
    if not torch.is_tensor(x) or x.dtype != dtype or not x.is_cuda or not x.is_contiguous() or \
            not (x.dim() == 3 or (x.dim() == 4 and x.shape[0] == 1)) or x.shape[c] != 3:
        raise ValueError(f"{what}: the frame is a contiguous {shape} tensor on the GPU (no CPU fallback)")
    hw = [int(s) for s in x.shape[-3:]]
    del hw[c]
    return tuple(hw)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def yuv_to_rgb_u8(planes_or_flat, H, W, spec, out=None):
    """planes_or_flat: (y, u, v) uint8 device tensors of spec.plane_shapes(H, W), or one flat uint8 device tensor Y|U|V of
    spec.frame_bytes(H, W) bytes (a y4m frame).  Returns the uint8 [H, W, 3] frame (`out`, if given: [H,W,3] or [1,H,W,3]).
    One launch on the current stream."""
    import torch
    from . import _lib
    _want(spec, YuvSpec, "yuv_to_rgb_u8")
    y, u, v = _device_planes(planes_or_flat, H, W, spec, "yuv_to_rgb_u8")
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=y.device)
    elif _frame_hw(out, "yuv_to_rgb_u8 out") != (H, W) or out.device != y.device:
        raise ValueError(f"out must be a uint8 [{H},{W},3] frame on {y.device}")
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().vst_yuv_to_rgb_u8(y.data_ptr(), u.data_ptr(), v.data_ptr(), H, W, *spec.codes, out.data_ptr(),
                                                _stream()), "vst_yuv_to_rgb_u8")
    return out


def rgb_to_yuv_u8(rgb, spec, out=None):
    """rgb: uint8 [H,W,3] (or [1,H,W,3]) device frame.  out: a flat uint8 device tensor of spec.frame_bytes(H, W) bytes or a
    (y, u, v) tuple of planes; default a new flat tensor.  Returns `out`.  One launch on the current stream."""
    import torch
    from . import _lib
    _want(spec, YuvSpec, "rgb_to_yuv_u8")
    H, W = _frame_hw(rgb, "rgb_to_yuv_u8")
    if out is None:
        out = torch.empty((spec.frame_bytes(H, W),), dtype=torch.uint8, device=rgb.device)
    y, u, v = _device_planes(out, H, W, spec, "rgb_to_yuv_u8 out")
    if y.device != rgb.device:
        raise ValueError("out must be on the frame's device")
    with torch.cuda.device(rgb.device):
        _lib.check(_lib.lib().vst_rgb_to_yuv_u8(rgb.data_ptr(), H, W, *spec.codes, y.data_ptr(), u.data_ptr(), v.data_ptr(),
                                                _stream()), "vst_rgb_to_yuv_u8")
    return out


def yuv16_to_rgb_f32(planes_or_flat, H, W, spec, out=None, out_u8=None):
    """planes_or_flat: (y, u, v) 16-bit device tensors of spec.plane_shapes(H, W), or one flat uint8 device tensor Y|U|V of
    spec.frame_bytes(H, W) bytes (a raw frame).  Returns the float32 [1, 3, H, W] planes on the 0..1 scale (`out`, if given).
    out_u8: a uint8 [H, W, 3] (or [1, H, W, 3]) device frame that receives the same pixels as bytes, floor(255 v + 0.5).  One
    launch on the current stream."""
    import torch
    from . import _lib
    _want(spec, DeepYuvSpec, "yuv16_to_rgb_f32")
    y, u, v = _device_planes(planes_or_flat, H, W, spec, "yuv16_to_rgb_f32")
    if out is None:
        out = torch.empty((1, 3, H, W), dtype=torch.float32, device=y.device)
    elif _frame_hw(out, "yuv16_to_rgb_f32 out", planar=True) != (H, W) or out.device != y.device:
        raise ValueError(f"out must be a float32 [1,3,{H},{W}] frame on {y.device}")
    if out_u8 is not None and (_frame_hw(out_u8, "yuv16_to_rgb_f32 out_u8") != (H, W) or out_u8.device != y.device):
        raise ValueError(f"out_u8 must be a uint8 [{H},{W},3] frame on {y.device}")
    lay, mat, rng, depth = spec.codes
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().vst_yuv16_to_rgb_f32(y.data_ptr(), u.data_ptr(), v.data_ptr(), H, W, depth, lay, mat, rng,
                                                   out.data_ptr(), None if out_u8 is None else out_u8.data_ptr(), _stream()),
                   "vst_yuv16_to_rgb_f32")
    return out if out.dim() == 4 else out[None]


def rgb_f32_to_yuv16(x, spec, out=None):
    """x: float32 [1, 3, H, W] (or [3, H, W]) device planes on the 0..1 scale.  out: a flat uint8 device tensor of
    spec.frame_bytes(H, W) bytes or a (y, u, v) tuple of 16-bit planes; default a new flat tensor.  Returns `out`.  One launch on
    the current stream."""
    import torch
    from . import _lib
    _want(spec, DeepYuvSpec, "rgb_f32_to_yuv16")
    H, W = _frame_hw(x, "rgb_f32_to_yuv16", planar=True)
    if out is None:
        out = torch.empty((spec.frame_bytes(H, W),), dtype=torch.uint8, device=x.device)
    y, u, v = _device_planes(out, H, W, spec, "rgb_f32_to_yuv16 out")
    if y.device != x.device:
        raise ValueError("out must be on the frame's device")
    lay, mat, rng, depth = spec.codes
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vst_rgb_f32_to_yuv16(x.data_ptr(), H, W, depth, lay, mat, rng, y.data_ptr(), u.data_ptr(),
                                                   v.data_ptr(), _stream()), "vst_rgb_f32_to_yuv16")
    return out


class DeepImgResize:
    """``img_resize`` in float for high-bit-depth frames of ONE source size, fused with yuv16_to_rgb_f32 (vstnet.h, "Deep resize";
    vst_yuv16_img_resize_f32): the 16-bit planes of an [H, W] frame in, the fp32 [1,3,h,w] planes at the stylised size out, and
    their u8 twin if asked for.  Tables and pass buffers are made up front and belong to this object, so one object serves one
    frame at a time (a pipeline keeps one per ring slot).  Raises VstError for a size outside the limits: sizes only shrink, a
    step by a factor of 16 at the most.  There is no host fallback."""

    def __init__(self, src_hw, spec, max_size, down_scale=4, device=None):
        import ctypes as C
        import torch
        from . import _lib
        from .resize import _tables_on, float_passes, img_resize_steps
        _want(spec, DeepYuvSpec, "DeepImgResize")
        self.src_hw, self.spec = (int(src_hw[0]), int(src_hw[1])), spec
        size_wh = (self.src_hw[1], self.src_hw[0])
        passes = float_passes(size_wh, max_size, down_scale)          # (raises for a size outside the limits)
        self.steps = img_resize_steps(size_wh, max_size, down_scale)
        self.size_wh = self.steps[-1] if self.steps else size_wh
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:           # ("cuda": the current device, by its index, as a tensor's device reads)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._steps = (C.c_int * max(1, 2 * len(self.steps)))(*[v for wh in self.steps for v in wh])
        nbytes = C.c_size_t(0)
        _lib.check(_lib.lib().vst_yuv16_img_resize_workspace_bytes(self.src_hw[0], self.src_hw[1], len(self.steps), self._steps,
                                                                   C.byref(nbytes)), "vst_yuv16_img_resize_workspace_bytes")
        with torch.cuda.device(self.device):
            self.tables = _tables_on("f64", self.device, [(a, b) for _, a, b in passes]) if passes else None
            self.work = torch.empty(nbytes.value // 4, dtype=torch.float32, device=self.device) if nbytes.value else None

    def __call__(self, planes_or_flat, out=None, out_u8=None):
        """planes_or_flat: as yuv16_to_rgb_f32 takes them, at the source size.  Returns the float32 [1, 3, h, w] planes (`out`, if
        given); out_u8: a uint8 [h, w, 3] (or [1, h, w, 3]) device frame for the twin.  Queued on the current stream."""
        import torch
        from . import _lib
        Hs, Ws = self.src_hw
        W, H = self.size_wh
        y, u, v = _device_planes(planes_or_flat, Hs, Ws, self.spec, "DeepImgResize")
        if y.device != self.device:
            raise ValueError(f"made for {self.device}, got planes on {y.device}")
        if out is None:
            out = torch.empty((1, 3, H, W), dtype=torch.float32, device=self.device)
        elif _frame_hw(out, "DeepImgResize out", planar=True) != (H, W) or out.device != self.device:
            raise ValueError(f"out must be a float32 [1,3,{H},{W}] frame on {self.device}")
        if out_u8 is not None and (_frame_hw(out_u8, "DeepImgResize out_u8") != (H, W) or out_u8.device != self.device):
            raise ValueError(f"out_u8 must be a uint8 [{H},{W},3] frame on {self.device}")
        lay, mat, rng, depth = self.spec.codes
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().vst_yuv16_img_resize_f32(
                y.data_ptr(), u.data_ptr(), v.data_ptr(), Hs, Ws, depth, lay, mat, rng, len(self.steps), self._steps,
                None if self.tables is None else self.tables.data_ptr(), None if self.work is None else self.work.data_ptr(),
                out.data_ptr(), None if out_u8 is None else out_u8.data_ptr(), _stream()), "vst_yuv16_img_resize_f32")
        return out if out.dim() == 4 else out[None]


def yuv16_img_resize_f32(planes_or_flat, Hs, Ws, spec, max_size, down_scale=4, out=None, out_u8=None):
    """``utils.utils.img_resize(frame, max_size, down_scale)`` in float of the high-bit-depth frame in planes_or_flat ((y, u, v)
    16-bit device tensors of spec.plane_shapes(Hs, Ws), or one flat uint8 device tensor): the float32 [1, 3, h, w] planes on the
    0..1 scale at the size resize.img_resize_size gives, and in out_u8 (uint8 [h, w, 3]) the same pixels as bytes.  One
    DeepImgResize made for the call (the tables are cached per device; the pass buffers are not)."""
    import torch
    planes = _planes(planes_or_flat, Hs, Ws, spec)
    device = planes[0].device if torch.is_tensor(planes[0]) else None
    return DeepImgResize((Hs, Ws), spec, max_size, down_scale, device)(planes_or_flat, out=out, out_u8=out_u8)
