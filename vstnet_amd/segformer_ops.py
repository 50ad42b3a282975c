"""The segmenter's kernels one by one (``vstnet_amd.segformer.ops``): thin wrappers of the kernel-level calls of
include/vstnet.h (vst_seg_gemm, ...), for tests and tools.

Every function takes contiguous float32 (or uint8 frame) CUDA tensors, queues one launch on torch's current stream and returns
``out``.  ``out`` may be a caller's tensor - a view into a larger buffer too, as long as it is contiguous and 16-byte aligned.
Maps are token-major [tokens, C].  The library refuses what it cannot run (``VstError``); there is no torch implementation
behind any of these.
"""
from __future__ import annotations

import ctypes as C

from . import _lib


def _f32(name, t, shape=None):
    import torch
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _out(out, shape, like):
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    return _f32("out", out, shape)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _call(name, like, *args):
    import torch
    with torch.cuda.device(like.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(getattr(_lib.lib(), name)(*args, st), name)


def gemm(a, w, bias=None, res=None, out=None):
    """out [M, N] = a [M, K] . w [N, K]^T (+ bias [N]) (+ res [M, N]); ``res`` may be ``out``."""
    _f32("a", a), _f32("w", w)
    (m, k), n = a.shape, w.shape[0]
    if a.dim() != 2 or w.dim() != 2 or w.shape[1] != k:
        raise ValueError(f"gemm: a {tuple(a.shape)} against w {tuple(w.shape)}")
    if bias is not None:
        _f32("bias", bias, (n,))
    if res is not None:
        _f32("res", res, (m, n))
    out = _out(out, (m, n), a)
    _call("vst_seg_gemm", a, _ptr(a), _ptr(w), _ptr(bias), _ptr(res), _ptr(out), m, n, k)
    return out


def layernorm(x, g, b, eps, out=None):
    """LayerNorm over the last axis of x [T, C] (C <= 512); ``out`` may be ``x``."""
    _f32("x", x)
    t, c = x.shape
    _f32("g", g, (c,)), _f32("b", b, (c,))
    out = _out(out, (t, c), x)
    _call("vst_seg_layernorm", x, _ptr(x), _ptr(g), _ptr(b), _ptr(out), t, c, float(eps))
    return out


def attention(q, kv, scale=0.125, out=None):
    """softmax(q k^T scale) v per head of 64 channels: q [N, C], kv [Nk, 2C] (K of head h at column 64 h, V at C + 64 h)."""
    _f32("q", q)
    n, c = q.shape
    _f32("kv", kv)
    if kv.dim() != 2 or kv.shape[1] != 2 * c:
        raise ValueError(f"attention: q {tuple(q.shape)} against kv {tuple(kv.shape)}")
    out = _out(out, (n, c), q)
    _call("vst_seg_attention", q, _ptr(q), _ptr(kv), _ptr(out), n, kv.shape[0], c, float(scale))
    return out


def dwconv_gelu(x, w, b, height, width, out=None):
    """GELU(depthwise 3x3 conv + b) of the height x width map x [height * width, C]; w [9, C] (tap-major)."""
    _f32("x", x)
    c = x.shape[1]
    _f32("x", x, (height * width, c)), _f32("w", w, (9, c)), _f32("b", b, (c,))
    out = _out(out, (height * width, c), x)
    _call("vst_seg_dwconv_gelu", x, _ptr(x), _ptr(w), _ptr(b), _ptr(out), int(height), int(width), c)
    return out


def im2col(x, height, width, k, stride, pad, out=None):
    """x [height * width, C] -> [Ho * Wo, k * k * C], the rows of a k x k conv's GEMM in the K order (ky, kx, c)."""
    _f32("x", x)
    c = x.shape[1]
    _f32("x", x, (height * width, c))
    ho, wo = (height + 2 * pad - k) // stride + 1, (width + 2 * pad - k) // stride + 1
    out = _out(out, (max(ho, 0) * max(wo, 0), k * k * c), x)
    _call("vst_seg_im2col", x, _ptr(x), int(height), int(width), c, int(k), int(stride), int(pad), _ptr(out))
    return out


def gather_rgb(frame_u8, out=None):
    """uint8 [H, W, 3] or [3, H, W] -> [h1 * w1, 147], the rows of patch_embed1's GEMM."""
    import torch
    f = frame_u8
    if not torch.is_tensor(f) or f.dtype != torch.uint8 or not f.is_cuda or not f.is_contiguous() or f.dim() != 3:
        raise ValueError("frame_u8 must be a contiguous uint8 CUDA tensor [H,W,3] or [3,H,W]")
    if 3 not in (f.shape[0], f.shape[2]):
        raise ValueError(f"expected [H,W,3] or [3,H,W], got {tuple(f.shape)}")
    chw = 0 if f.shape[2] == 3 else 1
    h, w = (f.shape[1], f.shape[2]) if chw else (f.shape[0], f.shape[1])
    hw8 = (C.c_int * 8)()
    _lib.check(_lib.lib().vst_seg_shape(int(h), int(w), hw8), "vst_seg_shape")
    h1, w1 = hw8[0], hw8[1]
    out = _out(out, (h1 * w1, 147), f)
    _call("vst_seg_gather_rgb", f, _ptr(f), chw, int(h), int(w), _ptr(out))
    return out


def head_sum(ys, grids, out=None):
    """ReLU(ys[0] + the bilinear upsamplings of ys[1..3] to grids[0]); ys[i] [h_i * w_i, E]; ``out`` may be ``ys[0]``."""
    if len(ys) != 4 or len(grids) != 4:
        raise ValueError("head_sum takes four maps and four grids")
    e = ys[0].shape[1]
    for y, (h, w) in zip(ys, grids):
        _f32("y", y, (h * w, e))
    out = _out(out, tuple(ys[0].shape), ys[0])
    hw8 = (C.c_int * 8)(*[int(v) for g in grids for v in g])
    _call("vst_seg_head_sum", ys[0], *[_ptr(y) for y in ys], hw8, e, _ptr(out))
    return out
