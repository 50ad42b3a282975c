"""Host-side helpers of the reference's inference scripts (reference: utils/utils.py:90-153), without the
torchvision dependency.  Only what image_transfer.py / video_transfer.py use."""
import os

import numpy as np
from PIL import Image

# label colours of hand-made segmentation maps, in the reference's dictionary order (utils/utils.py:106-116)
SEG_COLORS = [((0, 0, 255), 3), ((0, 255, 0), 2), ((0, 0, 0), 0), ((255, 255, 255), 1), ((255, 0, 0), 4),
              ((255, 255, 0), 5), ((128, 128, 128), 6), ((0, 255, 255), 7), ((255, 0, 255), 8)]


def img_resize(img, max_size, down_scale=None):
    """utils/utils.py:90-101 — bicubic shrink so the long edge is <= max_size, then floor both edges to a
    multiple of down_scale (a second bicubic resize)."""
    w, h = img.size
    if max(w, h) > max_size:
        w = int(1.0 * img.size[0] / max(img.size) * max_size)
        h = int(1.0 * img.size[1] / max(img.size) * max_size)
        img = img.resize((w, h), Image.BICUBIC)
    if down_scale is not None:
        w = w // down_scale * down_scale
        h = h // down_scale * down_scale
        img = img.resize((w, h), Image.BICUBIC)
    return img


def colors_to_labels(arr):
    """RGB [H,W,3] uint8 -> label map uint8 [H,W] (utils/utils.py:105-136): exact colour match, otherwise the
    colour with the smallest L1 distance; ties keep the earlier dictionary entry (the reference's tie branch
    raises inside a try/except and leaves the first minimum in place).  Vectorised instead of an O(HW) Python loop: the
    pixels are reduced to their DISTINCT colours first (a hand-made map has a handful; an anti-aliased one a few hundred), the
    nearest dictionary colour is found once per distinct colour and scattered back - a 1080p map takes ~40 ms instead of the
    0.4 s of a distance tensor over every pixel."""
    arr = np.asarray(arr)
    keys = np.array([c for c, _ in SEG_COLORS], dtype=np.int64)            # [9,3]
    vals = np.array([v for _, v in SEG_COLORS], dtype=np.uint8)
    packed = (arr[..., 0].astype(np.uint32) << 16) | (arr[..., 1].astype(np.uint32) << 8) | arr[..., 2].astype(np.uint32)
    out = np.empty(packed.shape, dtype=np.uint8)
    todo = np.ones(packed.shape, dtype=bool)
    for (r, g, b), v in SEG_COLORS:                                         # the exact matches: one compare per dictionary colour
        m = packed == ((r << 16) | (g << 8) | b)
        out[m] = v
        todo &= ~m
    if todo.any():                                                          # everything else: nearest colour per DISTINCT colour
        rest = packed[todo]
        uniq, inv = np.unique(rest, return_inverse=True)
        rgb = np.stack([(uniq >> 16) & 255, (uniq >> 8) & 255, uniq & 255], axis=-1).astype(np.int64)
        dist = np.abs(rgb[:, None, :] - keys[None, :, :]).sum(-1)           # [U,9]
        out[todo] = vals[np.argmin(dist, axis=-1)][inv]                      # argmin returns the first minimum
    return out


def load_segment(image_path, size=None):
    """utils/utils.py:104-153 — hand-made colour segmentation -> label map (optionally NEAREST-resized to size=(w,h))."""
    if not os.path.exists(image_path):
        print("Can not find image path: %s " % image_path)
        return None
    image = Image.open(image_path).convert("RGB")
    if size is not None:
        w, h = size
        image = image.resize((w, h), Image.NEAREST)
    image = np.array(image)
    if len(image.shape) == 3:
        image = colors_to_labels(image)
    return image


def to_tensor_u8(img):
    """PIL RGB image -> uint8 torch tensor [1,H,W,3] (the device side applies ToTensor's /255, RevResNet.forward_u8)."""
    import torch
    return torch.from_numpy(np.array(img.convert("RGB"), dtype=np.uint8))[None]       # (a writable copy: PIL's buffer is read-only)


def style_map_weights(planes):
    """The weights of --style_map / --style_maps from 8-bit grey planes at the code's resolution (uint8 [h, w] each), made in
    fp32: one plane is the weight of the second of two styles, t = v / 255 and w = (1 - t, t); K planes give
    w_k = v_k / sum_j v_j with the sum taken in integers.  float32 [K, h, w].  A pixel whose planes are all 0: ValueError."""
    planes = [np.asarray(p, dtype=np.uint8) for p in planes]
    if len(planes) == 1:
        t = planes[0].astype(np.float32) / np.float32(255.0)
        return np.stack([np.float32(1.0) - t, t])
    total = np.zeros(planes[0].shape, dtype=np.int32)
    for p in planes:
        if p.shape != planes[0].shape:
            raise ValueError("the planes of a style map have one size, got %s and %s" % (planes[0].shape, p.shape))
        total += p
    if (total == 0).any():
        y, x = (int(v) for v in np.argwhere(total == 0)[0])
        raise ValueError("every plane is 0 at pixel x = %d, y = %d (of the %dx%d weight grid): no style would be left there"
                         % (x, y, planes[0].shape[1], planes[0].shape[0]))
    tf = total.astype(np.float32)
    return np.stack([p.astype(np.float32) / tf for p in planes])
