"""The reference's import path for its perceptual losses (``from models.VGG import VGG19, calc_mean_std``), on the HIP kernels
of vstnet_amd/csrc/vgg.hip.  Inference only: nothing here records a gradient, and values come back as device float64.

``VGG19(checkpoint)`` takes the path of the reference's ``vgg_normalised.pth`` (a state dict with keys "0.weight" ...), such a
dict itself, or "synthetic".  Images are float32 [N,3,H,W] in [0,1] on the GPU; feature maps are [N,C,h,w] like the
reference's.  ``forward`` works from the encoder's per-tap records (vstnet_amd.vgg: one fused chain per image, no feature map
leaves the workspace except relu4_1 for the content loss).  The methods that hand out feature maps run the same kernels one
call at a time, on a packed copy of the weights that is made the first time one of them is called.
"""
import torch

from vstnet_amd import vgg as _vgg
from vstnet_amd.synth import VGG_CONVS, VGG_ENCODER_LAST, synthetic_vgg_state_dict

_TAP_CONVS = (2, 9, 16, 29)           # Sequential indices of the convs whose ReLU is relu1_1, relu2_1, relu3_1, relu4_1
_POOL_AFTER = (5, 12, 25)             # ... and of those whose ReLU (relu1_2, relu2_2, relu3_4) is followed by the max-pool


def _tokens(feat):
    """[C,h,w] -> contiguous token-major [h*w, C]"""
    return feat.reshape(feat.shape[0], -1).t().contiguous()


def _image(batch, i):
    return batch[i].float().contiguous()


def calc_mean_std(feat, eps=1e-5):
    """Per image and channel over the map: the mean and sqrt(unbiased variance + eps), each float64 [N,C,1,1]."""
    if feat.dim() != 4:
        raise ValueError(f"expected feature maps [N,C,h,w], got {tuple(feat.shape)}")
    n, c = feat.shape[:2]
    rec = torch.stack([_vgg.mean_std(_tokens(feat[i].float()), eps) for i in range(n)])          # [N,2,C]
    return rec[:, 0].reshape(n, c, 1, 1), rec[:, 1].reshape(n, c, 1, 1)


def _records_loss(rec_a, rec_b, levels):
    """the style loss of two record sets over their first `levels` taps, in fp64 on the device"""
    total = 0
    for (mean_a, std_a), (mean_b, std_b) in list(zip(_vgg.split_records(rec_a), _vgg.split_records(rec_b)))[:levels]:
        total = total + torch.mean((mean_a - mean_b) ** 2) + torch.mean((std_a - std_b) ** 2)
    return total


class VGG19(torch.nn.Module):
    def __init__(self, checkpoint="synthetic", device=None):
        super().__init__()
        if isinstance(checkpoint, str):
            checkpoint = synthetic_vgg_state_dict() if checkpoint == "synthetic" else torch.load(checkpoint, map_location="cpu")
        self.encoder = _vgg.VGGEncoder(checkpoint, device)
        self.device = self.encoder.device
        self._state = {k: v for k, v in checkpoint.items() if k.split(".")[0].isdigit() and int(k.split(".")[0]) <= VGG_ENCODER_LAST}
        self._packed = None

    def _layers(self):
        """(w9, b3, [(index, weight [Cout][9 Cin], bias)]) as the kernel-level calls take them, made on first use"""
        if self._packed is None:
            sd, dev = self._state, self.device
            convs = []
            for idx, cin, cout in VGG_CONVS[1:]:
                if idx > VGG_ENCODER_LAST:
                    break
                w = sd[f"{idx}.weight"].float().permute(0, 2, 3, 1)                 # K order (ky, kx, c)
                if cin % 4:
                    w = torch.nn.functional.pad(w, (0, 4 - cin % 4))                # the first conv: 3 -> 4 channels, zeros
                convs.append((idx, w.reshape(cout, -1).contiguous().to(dev), sd[f"{idx}.bias"].float().to(dev)))
            self._packed = (sd["0.weight"].float().reshape(9).to(dev), sd["0.bias"].float().to(dev), convs)
        return self._packed

    def _taps_of(self, img, n_layer):
        w9, b3, convs = self._layers()
        h, w = int(img.shape[1]), int(img.shape[2])
        x = _vgg.input_map(img, w9, b3)
        taps = []
        for idx, wt, b in convs:
            x = _vgg.conv3x3_relu(x, wt, b, h, w)
            if idx in _TAP_CONVS:
                taps.append(x.t().reshape(1, -1, h, w))
                if len(taps) == n_layer:
                    break
            if idx in _POOL_AFTER:
                x = _vgg.maxpool2(x, h, w)
                h, w = (h + 1) // 2, (w + 1) // 2
        return taps

    @torch.no_grad()
    def encode_with_intermediate(self, x, n_layer=4):
        """relu1_1 .. relu{n_layer}_1 of the images x [N,3,H,W], each float32 [N,C,h,w]"""
        if not 1 <= n_layer <= 4:
            raise ValueError("the encoder ends at relu4_1: n_layer is 1..4")
        per_image = [self._taps_of(_image(x, i), n_layer) for i in range(x.shape[0])]
        return [torch.cat(level) for level in zip(*per_image)]

    @torch.no_grad()
    def encode(self, x, n_layer=4):
        return self.encode_with_intermediate(x, n_layer)[-1]

    @torch.no_grad()
    def calc_content_loss(self, input, target):
        if input.shape != target.shape:
            raise ValueError(f"the content loss compares maps of one shape, got {tuple(input.shape)} and {tuple(target.shape)}")
        return _vgg.mse_f64(input.float().contiguous(), target.float().contiguous())[0]

    @torch.no_grad()
    def calc_style_loss(self, input, target):
        (mean_i, std_i), (mean_t, std_t) = calc_mean_std(input), calc_mean_std(target)
        return torch.mean((mean_i - mean_t) ** 2) + torch.mean((std_i - std_t) ** 2)

    @torch.no_grad()
    def forward(self, content_images, style_images, stylized_images, n_layer=4, content_weight=0):
        """-> (loss_c, loss_s), the reference's order: loss_s over relu1_1 .. relu{n_layer}_1 of the stylised images against
        the style images (as many as the stylised ones, or one for all), loss_c (0 unless content_weight > 0) on relu4_1
        against the content images.  Both are means over the batch."""
        n, n_style = stylized_images.shape[0], style_images.shape[0]
        want_content = content_weight > 0
        if not 1 <= n_layer <= 4:
            raise ValueError("the encoder ends at relu4_1: n_layer is 1..4")
        if want_content and n_layer < 4:
            raise ValueError("the content loss is taken on relu4_1: it needs n_layer = 4")
        if n_style not in (1, n):
            raise ValueError(f"{n_style} style images for {n} stylised images: pass as many, or one")
        if want_content and content_images.shape != stylized_images.shape:
            raise ValueError("the content loss needs content images of the stylised images' shape")
        meters = [_vgg.StyleLoss(self.encoder, _image(style_images, j)) for j in range(n_style)]
        loss_s = loss_c = 0
        for i in range(n):
            meter = meters[i % n_style]
            got = meter(_image(stylized_images, i), _image(content_images, i) if want_content else None).clone()
            # four taps: the library's own reduction; fewer: the same records, cut short
            loss_s = loss_s + (got[0] if n_layer == 4 else _records_loss(meter.records, meter.style_records, n_layer)) / n
            if want_content:
                loss_c = loss_c + got[1] / n
        return loss_c, loss_s
