"""The reference's import path for its Matting-Laplacian loss, on the device: ``compute_laplacian`` and ``laplacian_loss_grad``
with the reference's call sequence (train.py: ``M = compute_laplacian(img)``, later ``laplacian_loss_grad(stylized[i], M)``) and
its return values, without the HW x HW matrix.  The quadratic form collapses to a window stencil (vstnet_amd/matting.py,
csrc/matting.hip), so what ``compute_laplacian`` returns is a small handle that keeps the image, eps and win_rad."""
import numpy as np


class MattingHandle:
    """What compute_laplacian returns in place of the sparse matrix: the uint8 guide, eps, win_rad.  The guide is uploaded the
    first time the handle is used with an image, to that image's device."""

    def __init__(self, guide_u8, eps, win_rad):
        self.guide_u8, self.eps, self.win_rad = guide_u8, float(eps), int(win_rad)
        self._on = {}

    @property
    def shape(self):
        n = self.guide_u8.shape[0] * self.guide_u8.shape[1]
        return (n, n)                       # the matrix this stands for

    def guide_on(self, device):
        import torch
        if device not in self._on:
            self._on[device] = torch.from_numpy(self.guide_u8).to(device)
        return self._on[device]


def compute_laplacian(img, mask=None, eps=10 ** (-7), win_rad=1):
    """The Matting Laplacian of `img` (an [H,W,3] image with values 0..255, or the path of one) as a handle for
    laplacian_loss_grad."""
    if mask is not None:
        raise NotImplementedError("compute_laplacian(mask=...) is not supported: the loss is taken over every window of the image.")
    if isinstance(img, str):
        from PIL import Image
        img = Image.open(img).convert("RGB")
    a = np.asarray(img)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected an [H,W,3] image, got {a.shape}")
    if a.dtype != np.uint8:
        if not (np.all(a == np.round(a)) and a.min() >= 0 and a.max() <= 255):
            raise ValueError("the image must hold whole values in 0..255 (the device reads the guide as uint8)")
        a = a.astype(np.uint8)
    return MattingHandle(np.ascontiguousarray(a), eps, win_rad)


def laplacian_loss_grad(image, M):
    """The reference's pair for a [3,H,W] image on the GPU: the loss as a [1,1] tensor and 2.0 * gradient as [3,H,W], in the
    dtype and on the device of `image`."""
    import torch
    from vstnet_amd.matting import matting_loss
    if not torch.is_tensor(image) or not image.is_cuda:
        raise ValueError("image must be a tensor on the GPU (no CPU fallback)")
    if not isinstance(M, MattingHandle):
        raise TypeError("M must come from compute_laplacian")
    x = image.detach().to(torch.float32).contiguous()
    loss3, grad = matting_loss(M.guide_on(image.device), x, M.win_rad, M.eps, grad=True)
    return loss3.sum().reshape(1, 1).to(image.dtype), grad.to(image.dtype)
