"""High-bit-depth edge: 9..16-bit Y'CbCr planes <-> fp32 RGB planes on a 0..1 scale ("High-bit-depth edge").

Two pointwise HIP kernels (csrc/yuv16.hip: vst_yuv16_to_rgb_f32, vst_rgb_f32_to_yuv16) on device tensors, on the current stream:
a frame of headerless raw YUV (yuv420p10le, yuv422p10le, ...; vstnet_amd/rawyuv.py) goes up as the bytes it is on disk, enters
the encoder as float planes and leaves the decoder as float planes, so nothing between the file and the network passes through
256 levels.  There is no CPU path for those.  yuv16_to_rgb_host / rgb_to_yuv16_host state the same arithmetic in numpy float64
(include/vstnet.h has it in words): the tests' reference, and what `video_transfer.py --stub_stylise` rehearses with.  The 8-bit
edge (vstnet_amd/yuv.py) is a module of its own and does not change."""
from __future__ import annotations

import numpy as np

from .yuv import MATRICES, downsample_chroma, upsample_chroma

LAYOUTS = {"444": 0, "420jpeg": 1, "420mpeg2": 2, "422": 3}       # vstnet.h VST_YUV_444, _420_CENTRE, _420_LEFT, _422
RANGES = {"limited": 0, "full": 1}
DEPTHS = tuple(range(9, 17))
TIE_EPS = 2.0 ** -20     # the kernels' fp64 arithmetic errs by under 2^-32 of a code: a code may differ only this close to a tie


class DeepYuvSpec:
    """How a high-bit-depth frame's planes are laid out and what their codes mean: layout '444' | '422' (chroma on the even luma
    columns, every row) | '420jpeg' | '420mpeg2' (as YuvSpec), matrix 'bt601' | 'bt709', range 'limited' | 'full', depth 9..16
    bits in little-endian 16-bit samples."""

    def __init__(self, layout="420mpeg2", matrix="bt709", range="limited", depth=10):
        if layout not in LAYOUTS or matrix not in MATRICES or range not in RANGES or depth not in DEPTHS:
            raise ValueError(f"DeepYuvSpec: layout in {sorted(LAYOUTS)}, matrix in {sorted(MATRICES)}, range in {sorted(RANGES)}, "
                             f"depth in 9..16; got {layout!r}, {matrix!r}, {range!r}, {depth!r}")
        self.layout, self.matrix, self.range, self.depth = layout, matrix, range, int(depth)

    def __eq__(self, other):
        return isinstance(other, DeepYuvSpec) and self.codes == other.codes

    def __hash__(self):
        return hash(("deep",) + self.codes)

    def __repr__(self):
        return f"DeepYuvSpec({self.layout!r}, {self.matrix!r}, {self.range!r}, {self.depth})"

    @property
    def codes(self):
        """(layout, matrix, range, depth) as the library's enums and the depth"""
        return LAYOUTS[self.layout], MATRICES[self.matrix][0], RANGES[self.range], self.depth

    @property
    def max_code(self):
        return (1 << self.depth) - 1

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
        """bytes of one frame: two per sample"""
        y, c, _ = self.plane_shapes(H, W)
        return 2 * (y[0] * y[1] + 2 * c[0] * c[1])

    def split(self, flat, H, W):
        """The (y, u, v) views, in 16-bit samples, of one flat uint8 buffer Y|U|V (numpy array or torch tensor; a torch buffer
        must start on a 2-byte address).  numpy: '<u2' arrays.  torch: int16 tensors - the same 16 bits, there to be pointed at
        and copied, not computed with."""
        ys, cs, _ = self.plane_shapes(H, W)
        ny, nc = ys[0] * ys[1], cs[0] * cs[1]
        if flat.ndim != 1 or flat.shape[0] != 2 * (ny + 2 * nc) or (flat.dtype != np.uint8 if isinstance(flat, np.ndarray)
                                                                   else str(flat.dtype) != "torch.uint8"):
            raise ValueError(f"a {W}x{H} {self.layout} frame of {self.depth} bits is one flat uint8 buffer of {2 * (ny + 2 * nc)} "
                             f"bytes, got {flat.dtype} {tuple(flat.shape)}")
        if isinstance(flat, np.ndarray):
            s = flat.view("<u2")
        else:
            import torch
            s = flat.view(torch.int16)
        return s[:ny].reshape(ys), s[ny:ny + nc].reshape(cs), s[ny + nc:].reshape(cs)


# ---------------------------------------------------------------------------------------------------------------------------
# the arithmetic in float64
# ---------------------------------------------------------------------------------------------------------------------------
def near_tie(v, eps=TIE_EPS):
    """where v lies within eps of a rounding tie (x.5)"""
    v = np.asarray(v, np.float64)
    return np.abs((v - np.floor(v)) - 0.5) < eps


def round_codes(v, spec):
    """clamp(floor(v + 0.5), 0, 2^depth - 1) as uint16"""
    return np.clip(np.floor(np.asarray(v, np.float64) + 0.5), 0, spec.max_code).astype(np.uint16)


def _planes(planes_or_flat, H, W, spec):
    if isinstance(planes_or_flat, (tuple, list)):
        y, u, v = planes_or_flat
        for name, p, s in zip("yuv", (y, u, v), spec.plane_shapes(H, W)):
            if tuple(p.shape) != s:
                raise ValueError(f"plane {name} of a {W}x{H} {spec.layout} frame is {s}, got {tuple(p.shape)}")
        return y, u, v
    return spec.split(planes_or_flat, H, W)


def _upsample_422(plane, W):
    """a 4:2:2 plane sampled at every luma column: the chroma coordinate of luma x is x / 2, neighbours clamped"""
    p = np.asarray(plane, np.float64)
    x = np.arange(W)
    a, b = x // 2, np.minimum(x // 2 + 1, p.shape[1] - 1)
    w = (x % 2) * 0.5
    return (1 - w) * p[:, a] + w * p[:, b]


def _downsample_422(c):
    """float [H, W] chroma -> [H, ceil(W/2)]: [1/4, 1/2, 1/4] around the even column; a missing neighbour is the edge sample"""
    c = np.asarray(c, np.float64)
    W = c.shape[1]
    j = 2 * np.arange((W + 1) // 2)
    return 0.25 * c[:, np.maximum(j - 1, 0)] + 0.5 * c[:, j] + 0.25 * c[:, np.minimum(j + 1, W - 1)]


def yuv16_to_rgb_float(planes_or_flat, H, W, spec):
    """the unrounded R, G, B of every pixel on the 0..1 scale, clamped to [0, 1]: float64 [H, W, 3]"""
    def codes(p):           # (an int16 plane is a torch view of the same 16 bits); a code is first limited to 2^depth - 1
        p = np.asarray(p)
        return np.minimum((p.view(np.uint16) if p.dtype == np.int16 else p).astype(np.float64), spec.max_code)
    y, u, v = (codes(p) for p in _planes(planes_or_flat, H, W, spec))
    _, kr, kb = MATRICES[spec.matrix]
    yoff, ys, coff, cs = spec.scales
    kg = 1.0 - kr - kb
    if spec.layout == "422":
        u, v = _upsample_422(u, W), _upsample_422(v, W)
    elif spec.layout != "444":
        u, v = upsample_chroma(u, H, W, spec.layout), upsample_chroma(v, H, W, spec.layout)
    yy = (y - yoff) / ys
    pb, pr = (u - coff) / cs, (v - coff) / cs
    r = yy + 2 * (1 - kr) * pr
    b = yy + 2 * (1 - kb) * pb
    g = yy - (2 * (1 - kr) * kr / kg) * pr - (2 * (1 - kb) * kb / kg) * pb
    return np.clip(np.stack([r, g, b], axis=-1), 0.0, 1.0)


def yuv16_to_rgb_host(planes_or_flat, H, W, spec):
    """(float32 [H, W, 3] on the 0..1 scale, uint8 [H, W, 3] = floor(255 v + 0.5)): what the kernel's two outputs hold"""
    v = yuv16_to_rgb_float(planes_or_flat, H, W, spec)
    return v.astype(np.float32), np.floor(255.0 * v + 0.5).astype(np.uint8)


def rgb_to_yuv16_float(rgb, spec):
    """rgb: [H, W, 3] on the 0..1 scale (clamped here).  The unrounded codes of the three planes, one flat float64 array Y|U|V"""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected an [H, W, 3] frame, got {tuple(rgb.shape)}")
    _, kr, kb = MATRICES[spec.matrix]
    yoff, ys, coff, cs = spec.scales
    kg = 1.0 - kr - kb
    r, g, b = (np.clip(rgb[..., k].astype(np.float64), 0.0, 1.0) for k in range(3))
    y = kr * r + kg * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if spec.layout == "422":
        cb, cr = _downsample_422(cb), _downsample_422(cr)
    elif spec.layout != "444":
        cb, cr = downsample_chroma(cb, spec.layout), downsample_chroma(cr, spec.layout)
    return np.concatenate([(yoff + y * ys).reshape(-1), (coff + cb * cs).reshape(-1), (coff + cr * cs).reshape(-1)])


def rgb_to_yuv16_host(rgb, spec):
    """flat uint8 Y|U|V, two bytes per sample, little-endian (spec.split gives the planes)"""
    return round_codes(rgb_to_yuv16_float(rgb, spec), spec).astype("<u2").view(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# the device calls
# ---------------------------------------------------------------------------------------------------------------------------
def _device_planes(planes_or_flat, H, W, spec, what):
    import torch
    planes = _planes(planes_or_flat, H, W, spec)
    for p in planes:
        if not torch.is_tensor(p) or p.element_size() != 2 or p.is_floating_point() or not p.is_cuda or not p.is_contiguous() \
                or p.data_ptr() % 2:
            raise ValueError(f"{what}: the planes are contiguous 16-bit integer tensors on the GPU, or one flat uint8 tensor on a "
                             "2-byte address (no CPU fallback)")
    return planes


def _float_frame(x, what):
    import torch
    if not torch.is_tensor(x) or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or \
            not (x.dim() == 3 or (x.dim() == 4 and x.shape[0] == 1)) or x.shape[-3] != 3:
        raise ValueError(f"{what}: the frame is a contiguous float32 [1,3,H,W] (or [3,H,W]) tensor on the GPU (no CPU fallback)")
    return int(x.shape[-2]), int(x.shape[-1])


def yuv16_to_rgb_f32(planes_or_flat, H, W, spec, out=None, out_u8=None):
    """planes_or_flat: (y, u, v) 16-bit device tensors of spec.plane_shapes(H, W), or one flat uint8 device tensor Y|U|V of
    spec.frame_bytes(H, W) bytes (a raw frame).  Returns the float32 [1, 3, H, W] planes on the 0..1 scale (`out`, if given).
    out_u8: a uint8 [H, W, 3] (or [1, H, W, 3]) device frame that receives the same pixels as bytes, floor(255 v + 0.5).  One
    launch on the current stream."""
    import torch
    from . import _lib
    if not isinstance(spec, DeepYuvSpec):
        raise ValueError("yuv16_to_rgb_f32 takes a DeepYuvSpec")
    y, u, v = _device_planes(planes_or_flat, H, W, spec, "yuv16_to_rgb_f32")
    if out is None:
        out = torch.empty((1, 3, H, W), dtype=torch.float32, device=y.device)
    elif _float_frame(out, "yuv16_to_rgb_f32 out") != (H, W) or out.device != y.device:
        raise ValueError(f"out must be a float32 [1,3,{H},{W}] frame on {y.device}")
    if out_u8 is not None:
        from .yuv import _frame_hw
        if _frame_hw(out_u8, "yuv16_to_rgb_f32 out_u8") != (H, W) or out_u8.device != y.device:
            raise ValueError(f"out_u8 must be a uint8 [{H},{W},3] frame on {y.device}")
    lay, mat, rng, depth = spec.codes
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().vst_yuv16_to_rgb_f32(y.data_ptr(), u.data_ptr(), v.data_ptr(), H, W, depth, lay, mat, rng,
                                                   out.data_ptr(), None if out_u8 is None else out_u8.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), "vst_yuv16_to_rgb_f32")
    return out if out.dim() == 4 else out[None]


def rgb_f32_to_yuv16(x, spec, out=None):
    """x: float32 [1, 3, H, W] (or [3, H, W]) device planes on the 0..1 scale.  out: a flat uint8 device tensor of
    spec.frame_bytes(H, W) bytes or a (y, u, v) tuple of 16-bit planes; default a new flat tensor.  Returns `out`.  One launch on
    the current stream."""
    import torch
    from . import _lib
    if not isinstance(spec, DeepYuvSpec):
        raise ValueError("rgb_f32_to_yuv16 takes a DeepYuvSpec")
    H, W = _float_frame(x, "rgb_f32_to_yuv16")
    if out is None:
        out = torch.empty((spec.frame_bytes(H, W),), dtype=torch.uint8, device=x.device)
    y, u, v = _device_planes(out, H, W, spec, "rgb_f32_to_yuv16 out")
    if y.device != x.device:
        raise ValueError("out must be on the frame's device")
    lay, mat, rng, depth = spec.codes
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vst_rgb_f32_to_yuv16(x.data_ptr(), H, W, depth, lay, mat, rng, y.data_ptr(), u.data_ptr(),
                                                   v.data_ptr(), torch.cuda.current_stream().cuda_stream), "vst_rgb_f32_to_yuv16")
    return out
