"""Writes tests/golden/segformer_worksize.npz: the fp64 labels of frames segmented at a working resolution (--seg_size).

    python tests/make_segformer_worksize_golden.py

The reference is tests/segformer_ref.py, which tests/make_segformer_golden.py pins to the reference module at 1e-11; it needs no
reference checkout.  Per case: the frame is shrunk with PIL's 8-bit bicubic to ``SegFormer.work_hw`` (what
vstnet_amd.resize.resize_u8 reproduces byte for byte), the network runs on that working frame in fp64, and its quarter-resolution
logits are sampled with ONE F.interpolate(bilinear, align_corners=False) at the frame's own size; labels = argmax, margin = top-1
minus top-2 there.  ``e32`` is the error of an fp32 run of the same network against the fp64 run (max abs over max |logit|), the
unit of the GPU test's bound, as in make_segformer_golden.py.  A case is refused if more than 1 % of its pixels have a margin
under 2 * 8 * e32 * max|logit| or fewer than 4 labels hold >= 2 % of the pixels each.  Margins are stored as fp16 and labels as
uint8; the frames are not stored (the file stays under 1 MiB) but named by their scene seed, with a CRC-32 of their bytes.
"""
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import segformer_ref as R                                                             # noqa: E402
from vstnet_amd.segformer import SegFormer                                            # noqa: E402
from vstnet_amd.synth import synthetic_scene_u8, synthetic_segformer_state_dict      # noqa: E402

SEED = 4321
BOUND_FACTOR = 8
CASES = {      # name: (H, W, work_size, working (h, w), depths, scene seed)
    "up4": (288, 416, 104, (72, 104), (1, 1, 1, 1), 3),
    "ragged": (283, 409, 101, (70, 101), (1, 1, 1, 1), 5),
    "chain": (144, 208, 104, (72, 104), (2, 1, 2, 1), 2),
    "same": (96, 136, 136, (96, 136), (1, 1, 1, 1), 4),
}


def working_frame(frame, work_size):
    h, w = frame.shape[:2]
    hw, ww = SegFormer.work_hw(h, w, work_size)
    if (hw, ww) == (h, w):
        return frame
    return np.asarray(Image.fromarray(frame).resize((ww, hw), Image.BICUBIC))


def main():
    out = {}
    for name, (h, w, size, work_hw, depths, scene_seed) in CASES.items():
        sd = synthetic_segformer_state_dict(SEED, depths)
        frame = synthetic_scene_u8(h, w, scene_seed)
        work = working_frame(frame, size)
        assert work.shape[:2] == work_hw, (name, work.shape)
        with torch.no_grad():
            lg = R.segment(sd, work, depths, torch.float64)["logits"]
            lg32 = R.segment(sd, work, depths, torch.float32)["logits"]
            full = F.interpolate(lg[None], size=(h, w), mode="bilinear", align_corners=False)[0]
        labels = full.argmax(dim=0).to(torch.uint8)
        scale = float(lg.abs().max())
        e32 = float((lg32.double() - lg).abs().max()) / scale
        top = full.topk(2, dim=0).values
        margin = (top[0] - top[1]).numpy()
        threshold = 2 * BOUND_FACTOR * e32 * scale
        close = float((margin <= threshold).mean())
        _, counts = np.unique(labels.numpy(), return_counts=True)
        big = int((counts >= 0.02 * labels.numel()).sum())
        print(f"{name}: {h}x{w} at {work_hw[0]}x{work_hw[1]} depths {depths}: e32 {e32:.3e}, max|logit| {scale:.3f}, {big} labels "
              f">= 2 %, {100 * close:.4f} % of pixels under the margin threshold {threshold:.3e}")
        assert big >= 4, f"{name}: only {big} labels hold >= 2 % of the pixels"
        assert close <= 0.01, f"{name}: {close:.3%} of the pixels are closer than the comparison threshold"
        out[f"{name}.scene_seed"] = np.int64(scene_seed)           # the frame is synthetic_scene_u8(H, W, seed): too large to store
        out[f"{name}.frame_crc32"] = np.int64(zlib.crc32(frame.tobytes()))
        out[f"{name}.work_size"] = np.int64(size)
        out[f"{name}.work_hw"] = np.asarray(work_hw)
        out[f"{name}.depths"] = np.asarray(depths)
        out[f"{name}.labels"] = labels.numpy()
        out[f"{name}.margin"] = np.minimum(margin, 60000.0).astype(np.float16)
        out[f"{name}.e32"] = np.float64(e32)
        out[f"{name}.max_logit"] = np.float64(scale)
        out[f"{name}.share_close"] = np.float64(close)
        out[f"{name}.labels_2pct"] = np.int64(big)
    path = os.path.join(HERE, "golden", "segformer_worksize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
