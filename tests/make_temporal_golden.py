"""Writes tests/golden/temporal.npz: what the reference's own warp and TemporalLoss.forward give, on torch CPU, on small inputs.

    python tests/make_temporal_golden.py /path/to/reference

The reference's utils/TemporalLoss.py is imported by file path with an empty stand-in for cv2 in sys.modules first: it imports
cv2 at its top, and neither warp nor forward calls anything from it.  Cases: 8 x 8, 12 x 20 and 37 x 53, each with a real, an
integer, a zero and a larger-than-frame flow (tests/temporal_ref.py: make_flow; REAL_SCALE is the deviation of the real flows).

Recorded per case: the flow; the pixel every output pixel was read from, taken from the reference's warp of a frame whose three
planes hold the pixel's linear index, its row and its column (whole numbers below 2^24: exact in float32); and the loss of
forward(first, second, flow) on the two random frames recorded once per size, after checking that the warped frame forward
returns is the first frame read through that same index map.  Also the share of near-tie pixels per case (temporal_ref.near_tie),
which the GPU test bounds.  The tests read only the file."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import temporal_ref as R  # noqa: E402

GOLDEN_SIZES = R.SIZES[:3]
REAL_SCALE = 3.0


def main(ref_root):
    import torch
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_temporal", os.path.join(ref_root, "utils", "TemporalLoss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    loss_fn = ref.TemporalLoss()
    out = {"real_scale": np.float64(REAL_SCALE)}
    for h, w in GOLDEN_SIZES:
        yy, xx = np.mgrid[0:h, 0:w]
        index = np.stack([yy * w + xx, yy, xx]).astype(np.float32)
        first, second = R.make_frame_f32(h, w, 0), R.make_frame_f32(h, w, 1)
        out[f"{h}x{w}_first"], out[f"{h}x{w}_second"] = first, second
        for kind in R.FLOW_KINDS:
            flow = R.make_flow(h, w, kind)
            key = f"{h}x{w}_{kind}"
            warped = ref.warp(torch.from_numpy(index)[None], torch.from_numpy(flow)[None])[0].numpy()
            src = warped[0].astype(np.int32)
            assert np.array_equal(src, warped[1].astype(np.int32) * w + warped[2].astype(np.int32))
            loss, w_first = loss_fn(torch.from_numpy(first)[None], torch.from_numpy(second)[None], torch.from_numpy(flow)[None])
            assert np.array_equal(w_first[0].numpy(), first.reshape(3, -1)[:, src.ravel()].reshape(3, h, w))
            out[f"{key}_flow"], out[f"{key}_src"], out[f"{key}_loss"] = flow, src, np.float32(loss.item())
            out[f"{key}_near_tie"] = np.float64(R.near_tie(flow, h, w).mean())
            print(f"{key}: loss {loss.item():.9e}, near-tie share {out[f'{key}_near_tie']:.3e}")
    os.makedirs(os.path.join(HERE, "golden"), exist_ok=True)
    path = os.path.join(HERE, "golden", "temporal.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
