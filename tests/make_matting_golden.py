"""Writes tests/golden/matting.npz: what the reference's own Matting Laplacian gives on four small inputs.

    python tests/make_matting_golden.py /path/to/reference

The reference's utils/MattingLaplacian.py is imported by file path with an empty stand-in for cv2 in sys.modules first: the
ndarray, no-mask path calls nothing from cv2.  compute_laplacian builds the sparse matrix L (cast to float32, as the reference
returns it); the loss and 2 * gradient of laplacian_loss_grad are then taken with that float32 L multiplied in fp64, per
channel: grad = L x / (H W), loss = sum_c x_c . grad_c.  Recorded: the inputs (uint8 image, float32 x), win_rad, eps, the loss
and the doubled gradient.  Needs scipy; the tests read only the file."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def inputs():
    rng = np.random.default_rng(2024)
    noise = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    y, x = np.mgrid[0:16, 0:16]
    ramp = np.stack([12.0 * x + 20, 10.0 * y + 40, 5.0 * (x + y) + 30], 2)
    ramp = np.clip(ramp + rng.integers(-4, 5, (16, 16, 3)), 0, 255).astype(np.uint8)
    return {"noise": (noise, rng.random((3, 20, 24)).astype(np.float32)),
            "ramp": (ramp, rng.random((3, 16, 16)).astype(np.float32))}


def main(ref_root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_matting", os.path.join(ref_root, "utils", "MattingLaplacian.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"eps": np.float64(1e-7)}
    for name, (G, X) in inputs().items():
        out[f"{name}_guide"], out[f"{name}_x"] = G, X
        h, w = G.shape[:2]
        for r in (1, 2):
            L = ref.compute_laplacian(G, eps=1e-7, win_rad=r)
            assert L.dtype == np.float32
            L = L.tocsr().astype(np.float64)
            x = X.astype(np.float64).reshape(3, -1)
            grad = np.stack([L @ x[c] for c in range(3)]) / (h * w)
            out[f"{name}_r{r}_loss"] = np.float64((x * grad).sum())
            out[f"{name}_r{r}_grad2"] = (2.0 * grad).reshape(3, h, w)
            print(f"{name} r={r}: loss {out[f'{name}_r{r}_loss']:.12e}")
    os.makedirs(os.path.join(HERE, "golden"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "golden", "matting.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
