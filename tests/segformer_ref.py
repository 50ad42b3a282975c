"""Functional torch restatement of the segmenter (test infrastructure only): a forward over a ``SegmentModel`` state dict at
any dtype, written from the model's definition - overlapping patch embeddings, efficient self-attention with a
spatial-reduction conv, Mix-FFN with a depthwise conv, and the all-MLP decode head in its UNFOLDED form (four linears, three
upsamplings, concat, 1x1 fuse conv, eval BatchNorm, ReLU, prediction conv).  tests/make_segformer_golden.py checks it against
the reference implementation; the GPU code and the fp64 head fold are checked against it."""
import torch
import torch.nn.functional as F

DIMS = (64, 128, 320, 512)
HEADS = (1, 2, 5, 8)
SR = (8, 4, 2, 1)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _ln(x, sd, p, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + "weight"], sd[p + "bias"], eps)


def _attention(x, h, w, sd, p, heads, sr):
    n, c = x.shape
    q = F.linear(x, sd[p + "q.weight"], sd[p + "q.bias"]).reshape(n, heads, c // heads).transpose(0, 1)
    if sr > 1:
        m = x.t().reshape(1, c, h, w)
        m = F.conv2d(m, sd[p + "sr.weight"], sd[p + "sr.bias"], stride=sr).reshape(c, -1).t()
        x = _ln(m, sd, p + "norm.", 1e-5)
    kv = F.linear(x, sd[p + "kv.weight"], sd[p + "kv.bias"]).reshape(-1, 2, heads, c // heads)
    k, v = kv[:, 0].transpose(0, 1), kv[:, 1].transpose(0, 1)
    a = torch.softmax((q @ k.transpose(1, 2)) * (c // heads) ** -0.5, dim=-1)
    return F.linear((a @ v).transpose(0, 1).reshape(n, c), sd[p + "proj.weight"], sd[p + "proj.bias"])


def _mlp(x, h, w, sd, p):
    y = F.linear(x, sd[p + "fc1.weight"], sd[p + "fc1.bias"])
    c = y.shape[1]
    y = F.conv2d(y.t().reshape(1, c, h, w), sd[p + "dwconv.dwconv.weight"], sd[p + "dwconv.dwconv.bias"], padding=1, groups=c)
    y = F.gelu(y.reshape(c, -1).t())
    return F.linear(y, sd[p + "fc2.weight"], sd[p + "fc2.bias"])


def backbone(sd, x, depths):
    """x: [1,3,Hp,Wp] normalised -> [x1..x4], each [C_i, h_i, w_i]."""
    outs = []
    for s in range(4):
        k = 7 if s == 0 else 3
        p = f"backbone.patch_embed{s + 1}."
        x = F.conv2d(x, sd[p + "proj.weight"], sd[p + "proj.bias"], stride=4 if s == 0 else 2, padding=k // 2)
        _, c, h, w = x.shape
        t = _ln(x.reshape(c, -1).t(), sd, p + "norm.", 1e-5)
        for j in range(depths[s]):
            b = f"backbone.block{s + 1}.{j}."
            t = t + _attention(_ln(t, sd, b + "norm1.", 1e-6), h, w, sd, b + "attn.", HEADS[s], SR[s])
            t = t + _mlp(_ln(t, sd, b + "norm2.", 1e-6), h, w, sd, b + "mlp.")
        t = _ln(t, sd, f"backbone.norm{s + 1}.", 1e-6)
        x = t.t().reshape(1, c, h, w)
        outs.append(x[0])
    return outs


def decode_head(sd, xs):
    """The unfolded head: [x1..x4] -> quarter-resolution logits [150, h1, w1]."""
    size = xs[0].shape[1:]
    parts = []
    for i in (4, 3, 2, 1):
        x = xs[i - 1]
        y = F.linear(x.reshape(x.shape[0], -1).t(), sd[f"decode_head.linear_c{i}.proj.weight"], sd[f"decode_head.linear_c{i}.proj.bias"])
        y = y.t().reshape(1, -1, x.shape[1], x.shape[2])
        if i != 1:
            y = F.interpolate(y, size=size, mode="bilinear", align_corners=False)
        parts.append(y)
    p = "decode_head.linear_fuse."
    y = F.conv2d(torch.cat(parts, dim=1), sd[p + "conv.weight"])
    y = F.batch_norm(y, sd[p + "bn.running_mean"], sd[p + "bn.running_var"], sd[p + "bn.weight"], sd[p + "bn.bias"], False, 0.0, 1e-5)
    return F.conv2d(F.relu(y), sd["decode_head.linear_pred.weight"], sd["decode_head.linear_pred.bias"])[0]


def folded_head(folded, sd, xs):
    """The head as the device runs it, from ``vstnet_amd.segformer.fold_decode_head``'s fp64 result (torch tensors)."""
    size = xs[0].shape[1:]
    acc = None
    for i in (1, 2, 3, 4):
        x = xs[i - 1]
        y = (folded[f"fold_c{i}.weight"] @ x.reshape(x.shape[0], -1)).reshape(1, -1, x.shape[1], x.shape[2])
        if i == 1:
            acc = y + folded["fold.bias"].reshape(1, -1, 1, 1)
        else:
            acc = acc + F.interpolate(y, size=size, mode="bilinear", align_corners=False)
    return F.conv2d(F.relu(acc), sd["decode_head.linear_pred.weight"], sd["decode_head.linear_pred.bias"])[0]


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def segment(sd, frame_u8, depths, dtype=torch.float64):
    """frame_u8: uint8 [H,W,3] (numpy or torch) -> dict(xs, logits [150,hq,wq], full [150,H,W], labels uint8 [H,W])."""
    sd = cast(sd, dtype)
    f = torch.as_tensor(frame_u8).permute(2, 0, 1)[None].to(dtype) / 255.0
    _, _, h, w = f.shape
    f = F.pad(f, (0, (4 - w % 4) % 4, 0, (4 - h % 4) % 4), mode="replicate")
    mean = torch.tensor(MEAN, dtype=dtype).reshape(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype).reshape(1, 3, 1, 1)
    xs = backbone(sd, (f - mean) / std, depths)
    lg = decode_head(sd, xs)
    full = F.interpolate(lg[None], size=(h, w), mode="bilinear", align_corners=False)[0]
    return {"xs": xs, "logits": lg, "full": full, "labels": full.argmax(dim=0).to(torch.uint8)}
