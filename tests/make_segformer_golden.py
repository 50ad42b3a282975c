"""Writes tests/golden/segformer.npz, segformer_logits.npz and segformer_large.npz (build machine only: needs the reference
checkout).

    python tests/make_segformer_golden.py /path/to/reference

The reference's project/image_style/segment.py is imported by file path (torchvision's ``normalize`` and ``pdb`` are stubbed:
neither is installed / wanted here), a depth-[1,1,1,1] ``SegmentModel`` is built without ``__init__``'s checkpoint load, the
synthetic state dict is loaded, and the model runs in fp64 and in fp32 on the CPU.  tests/segformer_ref.py must equal it to
fp64 noise.  ``e32`` - the reference's own fp32 error against its fp64 run, max abs over max |logit| - is what the GPU tests'
bounds are built from.  The fixtures must not be degenerate: the script fails unless every label map has >= 4 labels holding
>= 2 % of the pixels each and <= 1 % of the pixels have a top-2 margin under the label test's threshold (2 * 8 * e32 * max|logit|).

Size limit: one committed file stays under 1 MiB, so the small case's full fp64 logits and the large case have files of their own.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import segformer_ref as R                                             # noqa: E402
from vstnet_amd.synth import (segformer_state_dict_spec, synthetic_scene_u8,          # noqa: E402
                              synthetic_segformer_state_dict)

SEED = 4321
BOUND_FACTOR = 8
CASES = {      # name: (H, W, depths, scene seed)
    "small": (72, 104, (1, 1, 1, 1), 0),
    "pad": (70, 101, (1, 1, 1, 1), 1),
    "chain": (72, 104, (2, 1, 2, 1), 2),
    "large": (264, 328, (1, 1, 1, 1), 3),
}


def load_reference(root):
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")

    def normalize(x, mean, std):
        m = torch.tensor(mean, dtype=x.dtype).reshape(1, 3, 1, 1)
        s = torch.tensor(std, dtype=x.dtype).reshape(1, 3, 1, 1)
        return (x - m) / s
    tvf.normalize = normalize
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf,
                        "pdb": types.ModuleType("pdb")})
    spec = importlib.util.spec_from_file_location("ref_segment", os.path.join(root, "project", "image_style", "segment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_model(mod, depths, sd, dtype):
    from functools import partial
    m = mod.SegmentModel.__new__(mod.SegmentModel)
    torch.nn.Module.__init__(m)
    m.MAX_TIMES = 4
    m.backbone = mod.VisionTransformer(patch_size=4, embed_dims=[64, 128, 320, 512], num_heads=[1, 2, 5, 8],
                                       mlp_ratios=[4, 4, 4, 4], norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                                       depths=list(depths), sr_ratios=[8, 4, 2, 1])
    m.decode_head = mod.SegFormerHead(768)
    m.num_classes = 150
    keys = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.load_state_dict(sd)
    return m.to(dtype).eval(), keys


def run_reference(m, frame_u8, dtype):
    """The model's forward with its intermediate results kept (same calls, same order as SegmentModel.forward)."""
    import torch.nn.functional as F
    x = torch.as_tensor(frame_u8).permute(2, 0, 1)[None].to(dtype) / 255.0
    _, _, h, w = x.shape
    labels = m(x)[0, 0].to(torch.uint8)
    xp = F.pad(x, (0, (4 - w % 4) % 4, 0, (4 - h % 4) % 4), mode="replicate")
    xp = sys.modules["torchvision.transforms.functional"].normalize(xp, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    xs = m.backbone(xp)
    lg = m.decode_head(xs)
    full = F.interpolate(lg, size=(h, w), mode="bilinear", align_corners=False)[0]
    assert torch.equal(full.argmax(0).to(torch.uint8), labels)
    return [t[0] for t in xs], lg[0], full, labels


def main(root):
    mod = load_reference(root)
    small, large, logits = {}, {}, {}
    for name, (h, w, depths, scene_seed) in CASES.items():
        sd = synthetic_segformer_state_dict(SEED, depths)
        frame = synthetic_scene_u8(h, w, scene_seed)
        with torch.no_grad():
            m64, keys = build_model(mod, depths, sd, torch.float64)
            assert keys == [(k, tuple(s)) for k, s in segformer_state_dict_spec(depths)], "state-dict spec differs from the model"
            xs, lg, full, labels = run_reference(m64, frame, torch.float64)
            m32, _ = build_model(mod, depths, sd, torch.float32)
            xs32, lg32, _, _ = run_reference(m32, frame, torch.float32)
            mine = R.segment(sd, frame, depths, torch.float64)
        scale = float(lg.abs().max())
        for a, b in zip(xs + [lg], mine["xs"] + [mine["logits"]]):
            assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(a.abs().max())), "segformer_ref.py differs from the reference"
        assert torch.equal(mine["labels"], labels)
        e32 = float((lg32.double() - lg).abs().max()) / scale
        e32_x = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(xs32, xs)]
        top = full.topk(2, dim=0).values
        margin = (top[0] - top[1]).numpy()
        threshold = 2 * BOUND_FACTOR * e32 * scale
        close = float((margin <= threshold).mean())
        _, counts = np.unique(labels.numpy(), return_counts=True)
        big = int((counts >= 0.02 * labels.numel()).sum())
        print(f"{name}: {h}x{w} depths {depths}: e32 {e32:.3e} (stages {['%.2e' % e for e in e32_x]}), max|logit| {scale:.3f}, "
              f"{big} labels >= 2 %, {100 * close:.4f} % of pixels under the margin threshold {threshold:.3e}")
        assert big >= 4, f"{name}: only {big} labels hold >= 2 % of the pixels"
        assert close <= 0.01, f"{name}: {close:.3%} of the pixels are closer than the comparison threshold"
        out = large if name == "large" else small
        out[f"{name}.frame"] = frame
        out[f"{name}.depths"] = np.asarray(depths)
        out[f"{name}.labels"] = labels.numpy()
        out[f"{name}.margin"] = np.minimum(margin, 60000.0).astype(np.float16)
        out[f"{name}.logits_s4"] = lg[:, ::4, ::4].numpy()
        out[f"{name}.e32"] = np.float64(e32)
        out[f"{name}.e32_stages"] = np.asarray(e32_x)
        out[f"{name}.max_logit"] = np.float64(scale)
        out[f"{name}.share_close"] = np.float64(close)
        out[f"{name}.labels_2pct"] = np.int64(big)
        if name == "small":
            for i, x in enumerate(xs):
                out[f"small.x{i + 1}"] = x.numpy()
            logits["small.logits"] = lg.numpy()
            out["keys"] = np.asarray([k for k, _ in keys])
            out["shapes"] = np.asarray([",".join(str(d) for d in s) for _, s in keys])
    gold = os.path.join(HERE, "golden")
    np.savez_compressed(os.path.join(gold, "segformer.npz"), **small)
    np.savez_compressed(os.path.join(gold, "segformer_large.npz"), **large)
    np.savez_compressed(os.path.join(gold, "segformer_logits.npz"), **logits)
    for f in ("segformer.npz", "segformer_large.npz", "segformer_logits.npz"):
        size = os.path.getsize(os.path.join(gold, f))
        print(f, size, "bytes")
        assert size < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
