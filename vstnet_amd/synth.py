"""Deterministic synthetic checkpoints and frames.

The reference's trained checkpoints (checkpoints/photo_image.pt, ...) are not
available offline, so every parity test, the smoke test and bench.py run on a
synthetic ``state_dict`` with exactly the reference's key names and shapes
(reference: models/RevResNet.py:68-94 residual_block, :119-129
channel_reduction, :166-201 RevResNet; SURVEY.md section 8(b) "State-dict
contract").  The generator is numpy-only so that the values do not depend on
the torch version, and biases are non-zero (the reference's default init zeroes
them, models/RevResNet.py:91-94, which would hide bias bugs).
"""
from __future__ import annotations

import numpy as np
import torch

# (stride, channel) of the 30 blocks of the stack, reference models/RevResNet.py:192-201
STACK = [(1, 16)] * 10 + [(2, 64)] + [(1, 64)] * 9 + [(2, 256)] + [(1, 256)] * 9
CONV_IDX = (1, 4, 7)  # positions of the Conv2d modules inside residual_block.conv


def block_conv_shapes(channel: int, stride: int, mult: int = 4):
    """OIHW shapes of the three convs of one residual_block (models/RevResNet.py:72-88)."""
    in_ch = channel if stride == 1 else channel // 4
    mid = channel // mult
    return [(mid, in_ch, 3, 3), (mid, mid, 3, 3), (channel, mid, 3, 3)]


def state_dict_spec(hidden_dim: int = 16, sp_steps: int = 2):
    """Ordered list of (key, shape) pairs — 192 tensors for both modes."""
    spec = []
    for i, (stride, ch) in enumerate(STACK):
        for ci, shp in zip(CONV_IDX, block_conv_shapes(ch, stride)):
            spec.append((f"stack.{i}.conv.{ci}.weight", shp))
            spec.append((f"stack.{i}.conv.{ci}.bias", (shp[0],)))
    cr_ch = hidden_dim * 4 ** sp_steps
    for i in range(2):
        for ci, shp in zip(CONV_IDX, block_conv_shapes(cr_ch, 1)):
            spec.append((f"channel_reduction.block_list.{i}.conv.{ci}.weight", shp))
            spec.append((f"channel_reduction.block_list.{i}.conv.{ci}.bias", (shp[0],)))
    return spec


def synthetic_state_dict(seed: int = 1234, hidden_dim: int = 16, sp_steps: int = 2,
                         weight_gain: float = 1.0, bias_scale: float = 0.05):
    """Seeded fp32 state_dict.  Weights ~ U(-g/sqrt(fan_in), g/sqrt(fan_in)), biases ~ U(-b, b)."""
    out = {}
    for idx, (key, shp) in enumerate(state_dict_spec(hidden_dim, sp_steps)):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if len(shp) == 4:
            bound = weight_gain / np.sqrt(shp[1] * shp[2] * shp[3])
        else:
            bound = bias_scale
        arr = rng.uniform(-bound, bound, size=shp).astype(np.float32)
        out[key] = torch.from_numpy(arr)
    return out


def synthetic_frames(batch: int, height: int, width: int, seed: int = 0) -> torch.Tensor:
    """[B,3,H,W] fp32 in [0,1): frame f is generated from (seed, f) so shards can make their own."""
    frames = []
    for f in range(batch):
        rng = np.random.Generator(np.random.PCG64([seed, f]))
        frames.append(rng.random((3, height, width), dtype=np.float32))
    return torch.from_numpy(np.stack(frames))


def synthetic_mask(height: int, width: int, labels: int = 5, seed: int = 0, speck: bool = True,
                   kind: str = "bands") -> np.ndarray:
    """uint8 [H,W] label map (+ one <=10-px speck of label `labels` that exercises the validity rule of
    models/cWCT.py:178).  kind "bands": vertical bands of `labels` labels; kind "noise": an independent uniform
    label per pixel — every 64-pixel tile holds every label, the worst case for per-label passes."""
    rng = np.random.Generator(np.random.PCG64([seed, 77]))
    if kind == "noise":
        m = rng.integers(0, labels, size=(height, width), dtype=np.uint8)
        if speck:
            m[1:3, 1:4] = labels
        return m
    if kind != "bands":
        raise ValueError("kind must be 'bands' or 'noise'")
    cuts = np.sort(rng.choice(np.arange(8, width - 8), size=labels - 1, replace=False))
    m = np.zeros((height, width), dtype=np.uint8)
    for i, c in enumerate(cuts):
        m[:, c:] = i + 1
    if speck:
        m[1:3, 1:4] = labels  # 6 pixels -> invalid label
    return m


# ------------------------------------------------------------------------------------------------ SegFormer (segmenter)
SEG_EMBED_DIMS = (64, 128, 320, 512)
SEG_SR_RATIOS = (8, 4, 2, 1)
SEG_CLASSES = 150
SEG_DEPTHS = {"b1": (2, 2, 2, 2), "b2": (3, 4, 6, 3), "b3": (3, 4, 18, 3), "b4": (3, 8, 27, 3), "b5": (3, 6, 40, 3)}


def segformer_state_dict_spec(depths=(3, 8, 27, 3), embedding_dim: int = 768):
    """Ordered (key, shape) pairs of the reference's ``SegmentModel`` state dict (project/image_style/segment.py: backbone =
    VisionTransformer :137-226, decode_head = SegFormerHead :391-426), in ``state_dict()`` order, without ``label_mapping``."""
    spec = []
    cin = 3
    for s, c in enumerate(SEG_EMBED_DIMS):
        k = 7 if s == 0 else 3
        p = f"backbone.patch_embed{s + 1}."
        spec += [(p + "proj.weight", (c, cin, k, k)), (p + "proj.bias", (c,)), (p + "norm.weight", (c,)), (p + "norm.bias", (c,))]
        cin = c
    for s, c in enumerate(SEG_EMBED_DIMS):
        sr = SEG_SR_RATIOS[s]
        for j in range(depths[s]):
            p = f"backbone.block{s + 1}.{j}."
            spec += [(p + "norm1.weight", (c,)), (p + "norm1.bias", (c,)),
                     (p + "attn.q.weight", (c, c)), (p + "attn.q.bias", (c,)),
                     (p + "attn.kv.weight", (2 * c, c)), (p + "attn.kv.bias", (2 * c,)),
                     (p + "attn.proj.weight", (c, c)), (p + "attn.proj.bias", (c,))]
            if sr > 1:
                spec += [(p + "attn.sr.weight", (c, c, sr, sr)), (p + "attn.sr.bias", (c,)),
                         (p + "attn.norm.weight", (c,)), (p + "attn.norm.bias", (c,))]
            spec += [(p + "norm2.weight", (c,)), (p + "norm2.bias", (c,)),
                     (p + "mlp.fc1.weight", (4 * c, c)), (p + "mlp.fc1.bias", (4 * c,)),
                     (p + "mlp.dwconv.dwconv.weight", (4 * c, 1, 3, 3)), (p + "mlp.dwconv.dwconv.bias", (4 * c,)),
                     (p + "mlp.fc2.weight", (c, 4 * c)), (p + "mlp.fc2.bias", (c,))]
        spec += [(f"backbone.norm{s + 1}.weight", (c,)), (f"backbone.norm{s + 1}.bias", (c,))]
    e = embedding_dim
    spec += [("decode_head.conv_seg.weight", (SEG_CLASSES, 128, 1, 1)), ("decode_head.conv_seg.bias", (SEG_CLASSES,))]
    for i in (4, 3, 2, 1):
        spec += [(f"decode_head.linear_c{i}.proj.weight", (e, SEG_EMBED_DIMS[i - 1])), (f"decode_head.linear_c{i}.proj.bias", (e,))]
    spec += [("decode_head.linear_fuse.conv.weight", (e, 4 * e, 1, 1)),
             ("decode_head.linear_fuse.bn.weight", (e,)), ("decode_head.linear_fuse.bn.bias", (e,)),
             ("decode_head.linear_fuse.bn.running_mean", (e,)), ("decode_head.linear_fuse.bn.running_var", (e,)),
             ("decode_head.linear_fuse.bn.num_batches_tracked", ()),
             ("decode_head.linear_pred.weight", (SEG_CLASSES, e, 1, 1)), ("decode_head.linear_pred.bias", (SEG_CLASSES,))]
    return spec


def synthetic_segformer_state_dict(seed: int = 4321, depths=(3, 8, 27, 3), embedding_dim: int = 768,
                                   weight_gain: float = 1.7, bias_scale: float = 0.1):
    """Seeded fp32 ``SegmentModel`` state dict, numpy-only and seeded per tensor.  Weights ~ U(-g/sqrt(fan_in), g/sqrt(fan_in))
    (g = sqrt(3) would keep the variance; the default is just under it), biases ~ U(-b, b) and never zero, LayerNorm / BatchNorm
    weights 1 + U(-0.1, 0.1), BN running mean U(-0.2, 0.2), running variance U(0.5, 1.5)."""
    out = {}
    for idx, (key, shp) in enumerate(segformer_state_dict_spec(depths, embedding_dim)):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if key.endswith("num_batches_tracked"):
            out[key] = torch.zeros((), dtype=torch.int64)
            continue
        if key.endswith("running_var"):
            arr = rng.uniform(0.5, 1.5, size=shp)
        elif key.endswith("running_mean"):
            arr = rng.uniform(-0.2, 0.2, size=shp)
        elif len(shp) >= 2:
            bound = weight_gain / np.sqrt(np.prod(shp[1:]))
            arr = rng.uniform(-bound, bound, size=shp)
        elif key.endswith("weight"):              # every 1-D weight is a LayerNorm's or the BatchNorm's
            arr = 1.0 + rng.uniform(-0.1, 0.1, size=shp)
        else:
            arr = rng.uniform(-bias_scale, bias_scale, size=shp)
        out[key] = torch.from_numpy(arr.astype(np.float32))
    return out


def synthetic_scene_u8(height: int, width: int, seed: int = 0) -> np.ndarray:
    """uint8 [H,W,3] test scene for the segmenter: a few large soft-edged colour regions with texture on top (pure noise gives
    every pixel the same features, hence one label everywhere)."""
    rng = np.random.Generator(np.random.PCG64([seed, 99]))
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    n = 6
    cy, cx = rng.uniform(0, height, n), rng.uniform(0, width, n)
    cols = rng.uniform(0, 255, (n, 3))
    d = np.stack([(yy - cy[i]) ** 2 + (xx - cx[i]) ** 2 for i in range(n)])
    w = np.exp(-d / (0.02 * (height * height + width * width)))
    w /= w.sum(0, keepdims=True)
    w = w ** 4
    w /= w.sum(0, keepdims=True)
    img = np.einsum("nhw,nc->hwc", w, cols)
    img += 25.0 * np.sin(yy / 3.1 + cx[0])[..., None] * np.cos(xx / 2.3)[..., None] + rng.normal(0, 6, (height, width, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ VGG-19 (style loss)
# (Sequential index, Cin, Cout) of every conv of the reference's build_vgg (models/VGG.py): the 1 x 1 conv, then the sixteen
# 3 x 3 convs of VGG-19.  The encoder of the style loss ends at relu4_1 (index 29); the rest is there so that the reference's
# own load_state_dict accepts the dict.
VGG_CONVS = ((0, 3, 3), (2, 3, 64), (5, 64, 64), (9, 64, 128), (12, 128, 128), (16, 128, 256), (19, 256, 256), (22, 256, 256),
             (25, 256, 256), (29, 256, 512), (32, 512, 512), (35, 512, 512), (38, 512, 512), (42, 512, 512), (45, 512, 512),
             (48, 512, 512), (51, 512, 512))
VGG_ENCODER_LAST = 29          # the conv in front of relu4_1


def vgg_state_dict_spec(full: bool = True):
    """Ordered (key, shape) pairs of build_vgg's state dict; full=False: only the layers up to relu4_1."""
    spec = []
    for idx, cin, cout in VGG_CONVS:
        if not full and idx > VGG_ENCODER_LAST:
            break
        k = 1 if idx == 0 else 3
        spec += [(f"{idx}.weight", (cout, cin, k, k)), (f"{idx}.bias", (cout,))]
    return spec


def synthetic_vgg_state_dict(seed: int = 1919):
    """Seeded fp32 stand-in for vgg_normalised.pth (not available offline), from ONE numpy RandomState drawn in layer order
    (weight, then bias): the 1 x 1 conv is I + 0.1 N(0, 1), a 3 x 3 conv N(0, 2 / (9 Cin)) (He: about half of every tap's
    activations stay positive through the nine layers), every bias 0.05 N(0, 1).  The values a style loss takes on these weights
    show that the instrument works and nothing more."""
    rng = np.random.RandomState(seed)
    out = {}
    for key, shp in vgg_state_dict_spec():
        if len(shp) == 1:
            arr = 0.05 * rng.standard_normal(shp)
        elif shp[2] == 1:
            arr = np.eye(3).reshape(shp) + 0.1 * rng.standard_normal(shp)
        else:
            arr = np.sqrt(2.0 / (9 * shp[1])) * rng.standard_normal(shp)
        out[key] = torch.from_numpy(arr.astype(np.float32))
    return out
