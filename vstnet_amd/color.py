"""Lab luminance-preserving post-process of the delldu fork (project/image_style/vstnet.py:189-220): keep the content
image's L channel, take a/b from the stylised image.  Pointwise HIP kernels (csrc/color.hip): vst_lab_luminance
on float images, vst_lab_luminance_u8[_f32] on the uint8 frames of the video loop; there is no CPU path."""
import torch

from . import _lib


def luminance_transfer(content: torch.Tensor, stylized: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """content, stylized: [B,3,H,W] fp32 on the same GPU, values in [0,1] (stylized is clamped like the fork's decoder
    output, vstnet.py:322).  Returns lab2rgb(cat(rgb2lab(content)[:, :1], rgb2lab(stylized)[:, 1:])) (color.py:94-113)."""
    if content.dim() != 4 or content.shape[1] != 3 or content.shape != stylized.shape:
        raise ValueError(f"expected two [B,3,H,W] tensors of equal shape, got {tuple(content.shape)} and {tuple(stylized.shape)}")
    if not content.is_cuda or content.device != stylized.device:
        raise RuntimeError("luminance_transfer runs on the GPU only (no CPU fallback)")
    content = content.float().contiguous()
    stylized = stylized.float().contiguous()
    if out is None:
        out = torch.empty_like(stylized)
    elif out.shape != stylized.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != content.device:
        raise ValueError("out must be a contiguous fp32 tensor shaped like the inputs on the same device")
    B, _, H, W = content.shape
    with torch.cuda.device(content.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().vst_lab_luminance(content.data_ptr(), stylized.data_ptr(), out.data_ptr(), B, H, W, stream),
                   "vst_lab_luminance")
    return out


def luminance_transfer_u8(content_u8: torch.Tensor, stylized: torch.Tensor, out: torch.Tensor = None,
                          to_float: bool = False) -> torch.Tensor:
    """The blend at the uint8 frame edge of the video loop.  content_u8: uint8 [B,H,W,3] device frames (what the frame loop
    holds; read as u8 / 255), stylized: [B,3,H,W] fp32 on the same GPU (a float decode).  Returns the blend quantised like
    inverse_u8, mul(255).clamp(0,255).byte() as uint8 [B,H,W,3] - or, to_float=True, as fp32 [B,3,H,W] for a resize to the writer
    size that comes after it (out may then be `stylized` itself).  One launch on the current stream (vst_lab_luminance_u8 /
    _u8_f32); there is no CPU path."""
    if content_u8.dim() != 4 or content_u8.shape[3] != 3 or content_u8.dtype != torch.uint8:
        raise ValueError(f"expected uint8 [B,H,W,3] content frames, got {content_u8.dtype} {tuple(content_u8.shape)}")
    B, H, W, _ = content_u8.shape
    if stylized.dim() != 4 or tuple(stylized.shape) != (B, 3, H, W):
        raise ValueError(f"expected a [{B},3,{H},{W}] stylised tensor for these frames, got {tuple(stylized.shape)}")
    if not content_u8.is_cuda or content_u8.device != stylized.device:
        raise RuntimeError("luminance_transfer_u8 runs on the GPU only (no CPU fallback)")
    content_u8 = content_u8.contiguous()
    stylized = stylized.float().contiguous()
    shape, dtype = ((B, 3, H, W), torch.float32) if to_float else ((B, H, W, 3), torch.uint8)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=stylized.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != stylized.device:
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on the same device")
    L = _lib.lib()
    fn, name = (L.vst_lab_luminance_u8_f32, "vst_lab_luminance_u8_f32") if to_float else (L.vst_lab_luminance_u8, "vst_lab_luminance_u8")
    with torch.cuda.device(stylized.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(fn(content_u8.data_ptr(), stylized.data_ptr(), out.data_ptr(), B, H, W, stream), name)
    return out
