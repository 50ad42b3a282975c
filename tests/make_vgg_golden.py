"""Writes tests/golden/vgg.npz: what the reference's own models/VGG.py returns, on torch CPU, for the cases of tests/vgg_ref.py.

    python tests/make_vgg_golden.py /path/to/reference

The reference's models/VGG.py is imported by file path.  Its VGG19 reads a checkpoint file with torch.load, so the synthetic
state dict (vstnet_amd.synth.synthetic_vgg_state_dict: vgg_normalised.pth is not available offline) is written to a temporary
file for it.  Recorded per case (frame, style, content: seeded uint8 images of tests/vgg_ref.py, as x / 255): loss_s and loss_c
of VGG19.forward(content, style, frame, content_weight=1) with the module at fp64 (.double()) and at fp32 on one thread, and the
frame's four mean / std records (calc_mean_std of encode_with_intermediate) at both precisions, laid out as the device lays
them out.  The weights and the images are stored as seeds, not as arrays; the key list of the reference's network is stored as
names.  tests/vgg_ref.py at fp64 must agree with the recorded fp64 values to 1e-12 (checked here and in tests/test_vgg_host.py).
The tests read only the file."""
import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vgg_ref as R  # noqa: E402


def main(ref_root):
    import torch
    spec = importlib.util.spec_from_file_location("ref_vgg", os.path.join(ref_root, "models", "VGG.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    sd = R.weights()
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "vgg_synthetic.pth")
        torch.save(sd, ckpt)
        nets = {"f64": ref.VGG19(ckpt).double().eval(), "f32": ref.VGG19(ckpt).eval()}
    out = {"weight_seed": np.int64(R.WEIGHT_SEED), "keys": np.array(list(ref.build_vgg().state_dict().keys())),
           "cases": np.array(sorted(R.CASES))}
    for case in sorted(R.CASES):
        frame, style, content = R.case_images(case)
        for prec, net in nets.items():
            dt = torch.float64 if prec == "f64" else torch.float32
            with torch.no_grad(), R.O.one_thread():
                loss_c, loss_s = net(R.planar(content, dt), R.planar(style, dt), R.planar(frame, dt), content_weight=1)
                rec = []
                for feat in net.encode_with_intermediate(R.planar(frame, dt)):
                    m, s = ref.calc_mean_std(feat)
                    rec += [m.reshape(-1), s.reshape(-1)]
            out[f"{case}.loss_s_{prec}"], out[f"{case}.loss_c_{prec}"] = np.float64(loss_s.item()), np.float64(loss_c.item())
            out[f"{case}.rec_{prec}"] = torch.cat(rec).double().numpy()
        mine = R.losses(frame, style, content, sd)
        for key in ("loss_s", "loss_c"):
            assert R.rel(mine[key], out[f"{case}.{key}_f64"]) <= 1e-12, (case, key)
        assert max(R.group_errs(mine["rec"], out[f"{case}.rec_f64"])) <= 1e-12, case
        print(f"{case}: loss_s {out[f'{case}.loss_s_f64']:.9e} (fp32 off by {R.rel(out[f'{case}.loss_s_f32'], out[f'{case}.loss_s_f64']):.2e}),"
              f" loss_c {out[f'{case}.loss_c_f64']:.9e} (fp32 off by {R.rel(out[f'{case}.loss_c_f32'], out[f'{case}.loss_c_f64']):.2e})")
    os.makedirs(os.path.join(HERE, "golden"), exist_ok=True)
    path = os.path.join(HERE, "golden", "vgg.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
