"""Raw video edge: 8-bit Y'CbCr planes <-> uint8 HWC RGB frames ("Raw video edge").

Two pointwise HIP kernels (csrc/yuv.hip: vst_yuv_to_rgb_u8, vst_rgb_to_yuv_u8) on device tensors, on the current stream - a
YUV4MPEG2 frame goes up and comes back as the 1.5 bytes per pixel it is on disk, and the conversion costs the frame's stream
one launch each way.  There is no CPU path for those.  yuv_to_rgb_host / rgb_to_yuv_host state the same arithmetic in numpy
float64 (include/vstnet.h has it in words): the tests' reference, and what `video_transfer.py --stub_stylise` rehearses with."""
from __future__ import annotations

import numpy as np

LAYOUTS = {"444": 0, "420jpeg": 1, "420mpeg2": 2}        # vstnet.h VST_YUV_444, VST_YUV_420_CENTRE, VST_YUV_420_LEFT
MATRICES = {"bt601": (0, 0.299, 0.114), "bt709": (1, 0.2126, 0.0722)}            # (VST_YUV_BT*, Kr, Kb)
RANGES = {"limited": (0, 16.0, 219.0, 224.0), "full": (1, 0.0, 255.0, 255.0)}    # (VST_YUV_*, Y offset, Y scale, chroma scale)
TIE_EPS = 2.0 ** -10     # the kernels' fp32 arithmetic errs by under 6e-5 on these magnitudes: a byte may differ only this close to a tie


class YuvSpec:
    """How a frame's planes are laid out and what their codes mean: layout '444' | '420jpeg' (chroma centred in its 2 x 2 luma
    block; y4m C420jpeg and C420) | '420mpeg2' (horizontally on the even luma columns; C420mpeg2), matrix 'bt601' | 'bt709',
    range 'limited' | 'full'."""

    def __init__(self, layout="420jpeg", matrix="bt601", range="limited"):
        if layout not in LAYOUTS or matrix not in MATRICES or range not in RANGES:
            raise ValueError(f"YuvSpec: layout in {sorted(LAYOUTS)}, matrix in {sorted(MATRICES)}, range in {sorted(RANGES)}; got "
                             f"{layout!r}, {matrix!r}, {range!r}")
        self.layout, self.matrix, self.range = layout, matrix, range

    def __eq__(self, other):
        return isinstance(other, YuvSpec) and self.codes == other.codes

    def __hash__(self):
        return hash(self.codes)

    def __repr__(self):
        return f"YuvSpec({self.layout!r}, {self.matrix!r}, {self.range!r})"

    @property
    def codes(self):
        """(layout, matrix, range) as the library's enums"""
        return LAYOUTS[self.layout], MATRICES[self.matrix][0], RANGES[self.range][0]

    def plane_shapes(self, H, W):
        """((H, W), chroma, chroma): chroma planes are ceil(H/2) x ceil(W/2) at 4:2:0"""
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"a frame is at least 1x1, got {W}x{H}")
        c = (H, W) if self.layout == "444" else ((H + 1) // 2, (W + 1) // 2)
        return (H, W), c, c

    def frame_bytes(self, H, W):
        y, c, _ = self.plane_shapes(H, W)
        return y[0] * y[1] + 2 * c[0] * c[1]

    def split(self, flat, H, W):
        """the (y, u, v) views of one flat Y|U|V buffer (numpy array or torch tensor)"""
        ys, cs, _ = self.plane_shapes(H, W)
        ny, nc = ys[0] * ys[1], cs[0] * cs[1]
        if flat.ndim != 1 or flat.shape[0] != ny + 2 * nc:
            raise ValueError(f"a {W}x{H} {self.layout} frame is one flat buffer of {ny + 2 * nc} bytes, got shape {tuple(flat.shape)}")
        return flat[:ny].reshape(ys), flat[ny:ny + nc].reshape(cs), flat[ny + nc:].reshape(cs)


# ---------------------------------------------------------------------------------------------------------------------------
# the arithmetic in float64
# ---------------------------------------------------------------------------------------------------------------------------
def round_bytes(v):
    """clamp(floor(v + 0.5), 0, 255) as uint8"""
    return np.clip(np.floor(np.asarray(v, np.float64) + 0.5), 0, 255).astype(np.uint8)


def near_tie(v, eps=TIE_EPS):
    """where v lies within eps of a rounding tie (x.5): the bytes the fp32 kernels may round the other way"""
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
    """a 4:2:0 plane sampled bilinearly at every luma position: float64 [H, W]"""
    p = np.asarray(plane, np.float64)
    ia, ib, wy = _taps(H, p.shape[0], True)
    ja, jb, wx = _taps(W, p.shape[1], layout == "420jpeg")
    top = (1 - wx) * p[ia][:, ja] + wx * p[ia][:, jb]
    bot = (1 - wx) * p[ib][:, ja] + wx * p[ib][:, jb]
    return (1 - wy)[:, None] * top + wy[:, None] * bot


def downsample_chroma(c, layout):
    """float [H, W] chroma -> float [ceil(H/2), ceil(W/2)]: rows averaged in pairs; columns in pairs ('420jpeg') or with
    [1/4, 1/2, 1/4] around the even column ('420mpeg2'); a missing neighbour is the edge sample again"""
    c = np.asarray(c, np.float64)
    H, W = c.shape
    j = 2 * np.arange((W + 1) // 2)
    if layout == "420jpeg":
        h = 0.5 * (c[:, j] + c[:, np.minimum(j + 1, W - 1)])
    else:
        h = 0.25 * c[:, np.maximum(j - 1, 0)] + 0.5 * c[:, j] + 0.25 * c[:, np.minimum(j + 1, W - 1)]
    i = 2 * np.arange((H + 1) // 2)
    return 0.5 * (h[i] + h[np.minimum(i + 1, H - 1)])


def _planes(planes_or_flat, H, W, spec):
    if isinstance(planes_or_flat, (tuple, list)):
        y, u, v = planes_or_flat
        shapes = spec.plane_shapes(H, W)
        for name, p, s in zip("yuv", (y, u, v), shapes):
            if tuple(p.shape) != s:
                raise ValueError(f"plane {name} of a {W}x{H} {spec.layout} frame is {s}, got {tuple(p.shape)}")
        return y, u, v
    return spec.split(planes_or_flat, H, W)


def yuv_to_rgb_float(planes_or_flat, H, W, spec):
    """the unrounded R, G, B of every pixel: float64 [H, W, 3]"""
    y, u, v = (np.asarray(p) for p in _planes(planes_or_flat, H, W, spec))
    _, kr, kb = MATRICES[spec.matrix]
    _, yoff, ys, cs = RANGES[spec.range]
    kg = 1.0 - kr - kb
    if spec.layout == "444":
        u, v = u.astype(np.float64), v.astype(np.float64)
    else:
        u, v = upsample_chroma(u, H, W, spec.layout), upsample_chroma(v, H, W, spec.layout)
    yy = (y.astype(np.float64) - yoff) * 255.0 / ys
    pb, pr = (u - 128.0) * 255.0 / cs, (v - 128.0) * 255.0 / cs
    r = yy + 2 * (1 - kr) * pr
    b = yy + 2 * (1 - kb) * pb
    g = yy - (2 * (1 - kr) * kr / kg) * pr - (2 * (1 - kb) * kb / kg) * pb
    return np.stack([r, g, b], axis=-1)


def yuv_to_rgb_host(planes_or_flat, H, W, spec):
    """uint8 [H, W, 3]"""
    return round_bytes(yuv_to_rgb_float(planes_or_flat, H, W, spec))


def rgb_to_yuv_float(rgb, spec):
    """the unrounded codes of the three planes, one flat float64 array Y|U|V"""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected an [H, W, 3] frame, got {tuple(rgb.shape)}")
    _, kr, kb = MATRICES[spec.matrix]
    _, yoff, ys, cs = RANGES[spec.range]
    kg = 1.0 - kr - kb
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    y = kr * r + kg * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if spec.layout != "444":
        cb, cr = downsample_chroma(cb, spec.layout), downsample_chroma(cr, spec.layout)
    return np.concatenate([(yoff + y * ys / 255.0).reshape(-1), (128.0 + cb * cs / 255.0).reshape(-1),
                           (128.0 + cr * cs / 255.0).reshape(-1)])


def rgb_to_yuv_host(rgb, spec):
    """flat uint8 Y|U|V (spec.split gives the planes)"""
    return round_bytes(rgb_to_yuv_float(rgb, spec))


# ---------------------------------------------------------------------------------------------------------------------------
# the device calls
# ---------------------------------------------------------------------------------------------------------------------------
def _device_planes(planes_or_flat, H, W, spec, what):
    import torch
    planes = _planes(planes_or_flat, H, W, spec)
    for p in planes:
        if not torch.is_tensor(p) or p.dtype != torch.uint8 or not p.is_cuda or not p.is_contiguous():
            raise ValueError(f"{what}: the planes are contiguous uint8 tensors on the GPU (no CPU fallback)")
    return planes


def _frame_hw(rgb, what):
    import torch
    if not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or not rgb.is_cuda or not rgb.is_contiguous() or \
            not (rgb.dim() == 3 or (rgb.dim() == 4 and rgb.shape[0] == 1)) or rgb.shape[-1] != 3:
        raise ValueError(f"{what}: the frame is a contiguous uint8 [H,W,3] (or [1,H,W,3]) tensor on the GPU (no CPU fallback)")
    return int(rgb.shape[-3]), int(rgb.shape[-2])


def yuv_to_rgb_u8(planes_or_flat, H, W, spec, out=None):
    """planes_or_flat: (y, u, v) uint8 device tensors of spec.plane_shapes(H, W), or one flat uint8 device tensor Y|U|V of
    spec.frame_bytes(H, W) bytes (a y4m frame).  Returns the uint8 [H, W, 3] frame (`out`, if given: [H,W,3] or [1,H,W,3]).
    One launch on the current stream."""
    import torch
    from . import _lib
    y, u, v = _device_planes(planes_or_flat, H, W, spec, "yuv_to_rgb_u8")
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=y.device)
    elif _frame_hw(out, "yuv_to_rgb_u8 out") != (H, W) or out.device != y.device:
        raise ValueError(f"out must be a uint8 [{H},{W},3] frame on {y.device}")
    lay, mat, rng = spec.codes
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().vst_yuv_to_rgb_u8(y.data_ptr(), u.data_ptr(), v.data_ptr(), H, W, lay, mat, rng, out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "vst_yuv_to_rgb_u8")
    return out


def rgb_to_yuv_u8(rgb, spec, out=None):
    """rgb: uint8 [H,W,3] (or [1,H,W,3]) device frame.  out: a flat uint8 device tensor of spec.frame_bytes(H, W) bytes or a
    (y, u, v) tuple of planes; default a new flat tensor.  Returns `out`.  One launch on the current stream."""
    import torch
    from . import _lib
    H, W = _frame_hw(rgb, "rgb_to_yuv_u8")
    if out is None:
        out = torch.empty((spec.frame_bytes(H, W),), dtype=torch.uint8, device=rgb.device)
    y, u, v = _device_planes(out, H, W, spec, "rgb_to_yuv_u8 out")
    if y.device != rgb.device:
        raise ValueError("out must be on the frame's device")
    lay, mat, rng = spec.codes
    with torch.cuda.device(rgb.device):
        _lib.check(_lib.lib().vst_rgb_to_yuv_u8(rgb.data_ptr(), H, W, lay, mat, rng, y.data_ptr(), u.data_ptr(), v.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "vst_rgb_to_yuv_u8")
    return out
