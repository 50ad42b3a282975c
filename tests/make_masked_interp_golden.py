"""Mints tests/golden/cwct_masked_interp.npz from the real reference (a CPU machine that has it; never the GPU machine):

    VST_REFERENCE=/path/to/reference python tests/make_masked_interp_golden.py

The reference's own ``cWCT.interpolation`` (models/cWCT.py:206-262) runs on the columns gathered per label, composed as
tests/masked_interp_ref.py composes the oracle's restatement.  Only data is written: inputs, label maps and outputs."""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests.masked_interp_ref import interpolation_seg_ref, region_mask  # noqa: E402


def reference_cwct():
    ref = os.environ.get("VST_REFERENCE")
    if not ref:
        raise SystemExit("set VST_REFERENCE to the reference checkout")
    import pdb
    pdb.set_trace = lambda *a, **k: None
    spec = importlib.util.spec_from_file_location("reference_cWCT", os.path.join(ref, "models", "cWCT.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.cWCT


def inputs():
    g = torch.Generator().manual_seed(2024)
    N = 32
    mixer = torch.eye(N) + 0.25 * torch.randn(N, N, generator=g)
    code = lambda h, w, k: (torch.einsum("ij,bjhw->bihw", mixer, torch.randn(1, N, h, w, generator=g)) * (0.5 + 0.2 * k) + 0.1 * k)
    c, sa, sb = code(24, 32, 0), code(16, 24, 1), code(12, 20, 2)
    cm = region_mask(24, 32, [0, 1, 2], 5)[None]
    sma = region_mask(16, 24, [0, 1, 2], 6)[None]
    smb = region_mask(12, 20, [0, 1], 7, tiny=2)[None]          # label 2: 6 pixels in style B -> valid against A, not B
    return c, sa, sb, cm, sma, smb


def main():
    cWCT = reference_cwct()
    c, sa, sb, cm, sma, smb = inputs()
    out = {"c": c.numpy(), "sa": sa.numpy(), "sb": sb.numpy(), "cm": cm, "sma": sma, "smb": smb,
           "alphas": np.array([0.6, 0.4], dtype=np.float64)}
    for ac in (0.0, 0.3):
        for dbl in (False, True):
            if dbl and ac == 0.0:
                continue
            ref = cWCT(use_double=dbl)
            o = interpolation_seg_ref(c, [sa, sb], [0.6, 0.4], ac, cm, [sma, smb],
                                      interp=lambda cc, ss, a, x: ref.interpolation(cc, ss, a, x))
            out["out_ac%s%s" % (ac, "_f64" if dbl else "")] = o.numpy()
    # both styles hold label 2: every label is mixed
    ref = cWCT()
    out["out_all_valid"] = interpolation_seg_ref(c, [sa, sa.flip(3)], [0.6, 0.4], 0.3, cm, [sma, sma[:, :, ::-1].copy()],
                                                 interp=lambda cc, ss, a, x: ref.interpolation(cc, ss, a, x)).numpy()
    path = os.path.join(REPO, "tests", "golden", "cwct_masked_interp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
