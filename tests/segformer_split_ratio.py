"""Host restatement of the segmenter's GEMM arithmetic (run by hand: `python tests/segformer_split_ratio.py`).

Every Linear / conv of tests/segformer_ref.py and the folded decode head is computed as the device GEMM computes it - operands
rounded to bf16 parts, one fp32 matmul per product kept - for the two-way split (bf16x3: hi.hi + hi.lo + lo.hi) and for the
three-way split csrc/segformer.hip uses (six products).  Prints, per fixture, the error of x1..x4 and of the logits against the
fp64 golden run as a multiple of e32, the reference's own fp32 error.  DESIGN.md ("On-device segmentation") quotes the output."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import segformer_ref as R                                             # noqa: E402
from vstnet_amd.segformer import fold_decode_head                      # noqa: E402
from vstnet_amd.synth import synthetic_segformer_state_dict            # noqa: E402


def parts(a, ways):
    out, r = [], a
    for _ in range(ways):
        p = r.to(torch.bfloat16).float()
        out.append(p)
        r = r - p
    return out


def split_mm(a, w, ways):
    """a [M,K] . w [N,K]^T with the products whose weight is above 2^(-8 ways): part i of a times part j of w for i + j < ways."""
    pa, pw = parts(a, ways), parts(w, ways)
    terms = sorted(((i + j, i, j) for i in range(ways) for j in range(ways) if i + j < ways), reverse=True)
    acc = None
    for _, i, j in terms:                  # smallest terms first
        t = pa[i] @ pw[j].t()
        acc = t if acc is None else acc + t
    return acc


def run(sd, frame, depths, ways):
    orig_linear, orig_conv = F.linear, F.conv2d

    def linear(x, w, b=None):
        y = split_mm(x, w, ways)
        return y if b is None else y + b

    def conv2d(x, w, b=None, stride=1, padding=0, groups=1):
        if groups != 1:
            return orig_conv(x, w, b, stride=stride, padding=padding, groups=groups)
        cols = F.unfold(x, w.shape[2:], padding=padding, stride=stride)[0].t()
        y = split_mm(cols, w.reshape(w.shape[0], -1), ways)
        y = y if b is None else y + b
        ho = (x.shape[2] + 2 * padding - w.shape[2]) // stride + 1
        return y.t().reshape(1, w.shape[0], ho, -1)
    sd32 = R.cast(sd, torch.float32)
    f = torch.as_tensor(frame).permute(2, 0, 1)[None].float() / 255
    mean, std = torch.tensor(R.MEAN).reshape(1, 3, 1, 1), torch.tensor(R.STD).reshape(1, 3, 1, 1)
    F.linear, F.conv2d = linear, conv2d
    try:
        xs = R.backbone(sd32, (f - mean) / std, depths)
    finally:
        F.linear, F.conv2d = orig_linear, orig_conv
    folded = {k: torch.from_numpy(v).float() for k, v in fold_decode_head(sd).items()}
    acc = None
    for i in (1, 2, 3, 4):
        x = xs[i - 1]
        y = split_mm(x.reshape(x.shape[0], -1).t(), folded[f"fold_c{i}.weight"], ways).t().reshape(1, -1, x.shape[1], x.shape[2])
        if i == 1:
            acc = y + folded["fold.bias"].reshape(1, -1, 1, 1)
        else:
            acc = acc + F.interpolate(y, size=xs[0].shape[1:], mode="bilinear", align_corners=False)
    a = F.relu(acc)[0]
    lg = split_mm(a.reshape(a.shape[0], -1).t(), sd32["decode_head.linear_pred.weight"].reshape(150, -1), ways)
    lg = (lg + sd32["decode_head.linear_pred.bias"]).t().reshape(150, *a.shape[1:])
    return xs, lg


def main():
    g = dict(np.load(os.path.join(HERE, "golden", "segformer.npz")))
    for case in ("small", "chain"):
        depths = tuple(int(d) for d in g[case + ".depths"])
        sd = synthetic_segformer_state_dict(4321, depths)
        with torch.no_grad():
            ref = R.segment(sd, g[case + ".frame"], depths, torch.float64)
            e32 = float(g[case + ".e32"])
            for ways in (2, 3):
                xs, lg = run(sd, g[case + ".frame"], depths, ways)
                errs = [float((x.double() - r).abs().max() / r.abs().max()) for x, r in zip(xs + [lg], ref["xs"] + [ref["logits"]])]
                print(f"{case} (depths {depths}), {ways}-way split: error / e32 of x1..x4, logits =", [round(e / e32, 2) for e in errs])


if __name__ == "__main__":
    main()
