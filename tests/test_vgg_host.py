"""Style loss, the parts that need no GPU: the reference statement against the golden file, the teeth of the GPU tests' bound,
every refusal of the C ABI (all returned before a launch, so they run without a device), the drop-in signatures of
models/VGG.py and the synthetic state dict against the key list of the reference's network."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import vgg_ref as R                                                    # noqa: E402

from vstnet_amd import _lib                                            # noqa: E402
from vstnet_amd.synth import synthetic_vgg_state_dict, vgg_state_dict_spec      # noqa: E402

ARG, SHAPE, WORKSPACE = -1, -2, -4
NEW_EXPORTS = ["vst_vgg_create", "vst_vgg_load_tensor", "vst_vgg_workspace_bytes", "vst_vgg_features_u8", "vst_vgg_features_f32",
               "vst_vgg_destroy", "vst_vgg_input_u8", "vst_vgg_input_f32", "vst_vgg_conv3x3_relu", "vst_vgg_maxpool2",
               "vst_vgg_mean_std_workspace_bytes", "vst_vgg_mean_std", "vst_vgg_mse_f64", "vst_vgg_style_loss"]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("vgg")


@pytest.fixture(scope="module")
def sd(gold):
    return R.weights(int(gold["weight_seed"]))


# ------------------------------------------------------------------------------------------------------------- golden
def test_reference_statement_matches_golden(gold, sd):
    assert sorted(R.CASES) == list(gold["cases"])
    for case in sorted(R.CASES):
        mine = R.losses(*R.case_images(case), sd)
        for key in ("loss_s", "loss_c"):
            assert R.rel(mine[key], gold[f"{case}.{key}_f64"]) <= 1e-12, (case, key)
        assert max(R.group_errs(mine["rec"], gold[f"{case}.rec_f64"])) <= 1e-12, case


def test_bound_has_teeth(gold, sd):
    """FACTOR by the project's rule: the fp32 restatement of the device arithmetic stays <= FACTOR / 2 on every case and every
    figure, and every mutant is >= 1.25 x FACTOR on at least one case."""
    worst = 0.0
    for case in sorted(R.CASES):
        r = R.ratios(R.losses(*R.case_images(case), sd, torch.float32, enc=R.encode_restated), gold, case)
        print(f"restatement {case}: " + ", ".join(f"{k} {v:.2f}" for k, v in r.items()))
        worst = max(worst, max(r.values()))
    assert worst <= R.FACTOR / 2, worst
    for mutant in R.MUTANTS:
        best = 0.0
        for case in sorted(R.CASES):
            try:
                r = R.ratios(R.losses(*R.case_images(case), sd, mutant=mutant), gold, case)
            except RuntimeError:          # floor pooling leaves a 1-pixel edge at 9 x 9, which torch's reflection refuses
                assert mutant == "floor pooling" and case == "9x9"
                continue
            best = max(best, max(r.values()))
        print(f"mutant {mutant!r}: {best:.3g} x max(e32, floor)")
        assert best >= 1.25 * R.FACTOR, (mutant, best)


def test_floor_and_e32(gold):
    """the floor is needed: at least one golden scalar has an fp32 error under 1 u (luck), none is above 64 u"""
    e = [R.rel(gold[f"{c}.{k}_f32"], gold[f"{c}.{k}_f64"]) for c in sorted(R.CASES) for k in ("loss_s", "loss_c")]
    print("e32 of the golden scalars:", ", ".join(f"{v:.2e}" for v in e))
    assert min(e) < R.U < R.FLOOR and max(e) < 64 * R.U


# -------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_spec_matches_reference_keys(gold):
    keys = [str(k) for k in gold["keys"]]
    assert [k for k, _ in vgg_state_dict_spec()] == keys
    enc = [k for k, _ in vgg_state_dict_spec(full=False)]
    assert enc == keys[:len(enc)] and enc[-1] == "29.bias" and len(enc) == 20
    a, b = synthetic_vgg_state_dict(7), synthetic_vgg_state_dict(7)
    assert list(a) == keys and all(torch.equal(a[k], b[k]) and a[k].dtype == torch.float32 for k in keys)
    assert not torch.equal(a["2.weight"], synthetic_vgg_state_dict(8)["2.weight"])
    assert tuple(a["0.weight"].shape) == (3, 3, 1, 1) and tuple(a["29.weight"].shape) == (512, 256, 3, 3)
    assert float((a["0.weight"].reshape(3, 3) - torch.eye(3)).abs().max()) < 0.6
    assert abs(float(a["19.weight"].std()) / (2.0 / (9 * 256)) ** 0.5 - 1) < 0.02 and abs(float(a["19.bias"].std()) / 0.05 - 1) < 0.2


def test_activations_and_losses_are_in_range(gold, sd):
    """what the synthetic rule is for: about half of every tap's activations positive, losses neither 0 nor huge"""
    with torch.no_grad():
        taps = R.encode(R.planar(R.case_images("32x48")[0], torch.float64), sd)
    for t in taps:
        assert 0.3 < float((t > 0).double().mean()) < 0.7
    for case in sorted(R.CASES):
        assert 1e-3 < float(gold[f"{case}.loss_s_f64"]) < 1.0 and 1e-3 < float(gold[f"{case}.loss_c_f64"]) < 1.0


# --------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_exports():
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(L, name), name
    assert f"#define VST_VGG_RECORD_DOUBLES {_lib.VGG_RECORD_DOUBLES}" in hdr
    assert f"#define VST_VGG_MSE_WS_BYTES {_lib.VGG_MSE_WS_BYTES}" in hdr
    assert _lib.VGG_RECORD_DOUBLES == 2 * sum(R.LEVEL_CHANNELS)
    # no scratch: the guard is _lib.build(), which refuses a library with a kernel that spills; the table it leaves next to the
    # library is read here only to see that the new kernels are in it (a library built elsewhere comes without the table)
    if os.path.exists(_lib.RESOURCES_PATH):
        lines = [ln for ln in open(_lib.RESOURCES_PATH).read().splitlines() if "vgg_" in ln and "ScratchSize" in ln]
        assert len(lines) >= 10 and any("vgg_conv_kernel" in ln for ln in lines)
        assert all(ln.rstrip().endswith(": 0") for ln in lines), lines


def test_abi_refusals():
    """host memory stands in for device memory: every call below returns before it launches or touches anything"""
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) // 64 * 64
    x, o, x4, x8 = base, base + 2048, base + 4, base + 8
    null, ws = None, base + 1024
    n = C.c_size_t(0)
    calls = [
        # input
        (ARG, L.vst_vgg_input_u8, (null, x, x, o, 4, 4, null)), (ARG, L.vst_vgg_input_u8, (x, null, x, o, 4, 4, null)),
        (ARG, L.vst_vgg_input_u8, (x, x, null, o, 4, 4, null)), (ARG, L.vst_vgg_input_u8, (x, x, x, null, 4, 4, null)),
        (ARG, L.vst_vgg_input_u8, (x, x, x, x4, 4, 4, null)), (ARG, L.vst_vgg_input_u8, (x, x + 2, x, o, 4, 4, null)),
        (SHAPE, L.vst_vgg_input_u8, (x, x, x, o, 0, 4, null)), (SHAPE, L.vst_vgg_input_u8, (x, x, x, o, 4, -1, null)),
        (SHAPE, L.vst_vgg_input_u8, (x, x, x, o, 4097, 4096, null)),
        (ARG, L.vst_vgg_input_f32, (null, x, x, o, 4, 4, null)), (ARG, L.vst_vgg_input_f32, (x + 2, x, x, o, 4, 4, null)),
        (ARG, L.vst_vgg_input_f32, (x, x, x, x8, 4, 4, null)), (SHAPE, L.vst_vgg_input_f32, (x, x, x, o, 4, 0, null)),
        (SHAPE, L.vst_vgg_input_f32, (x, x, x, o, 4096, 4097, null)),
        # conv: null / misaligned, Cin % 4, Cin < 4, Cout < 1, an edge under 2, oversize, overlap
        (ARG, L.vst_vgg_conv3x3_relu, (null, x, x, o, 2, 2, 4, 4, null)), (ARG, L.vst_vgg_conv3x3_relu, (x, null, x, o, 2, 2, 4, 4, null)),
        (ARG, L.vst_vgg_conv3x3_relu, (x, x, null, o, 2, 2, 4, 4, null)), (ARG, L.vst_vgg_conv3x3_relu, (x, x, x, null, 2, 2, 4, 4, null)),
        (ARG, L.vst_vgg_conv3x3_relu, (x4, x, x, o, 2, 2, 4, 4, null)), (ARG, L.vst_vgg_conv3x3_relu, (x, x8, x, o, 2, 2, 4, 4, null)),
        (ARG, L.vst_vgg_conv3x3_relu, (x, x, x4, o, 2, 2, 4, 4, null)), (ARG, L.vst_vgg_conv3x3_relu, (x, x, x, o + 4, 2, 2, 4, 4, null)),
        (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 2, 2, 6, 4, null)), (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 2, 2, 3, 4, null)),
        (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 2, 2, 0, 4, null)), (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 2, 2, 4, 0, null)),
        (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 1, 2, 4, 4, null)), (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 2, 1, 4, 4, null)),
        (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 4097, 4096, 4, 4, null)),
        (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 4096, 4096, 128, 4, null)),
        (SHAPE, L.vst_vgg_conv3x3_relu, (x, x, x, o, 4096, 4096, 4, 128, null)),
        (ARG, L.vst_vgg_conv3x3_relu, (x, o, o, x, 2, 2, 4, 4, null)), (ARG, L.vst_vgg_conv3x3_relu, (x, o, o, x + 48, 2, 2, 4, 4, null)),
        (ARG, L.vst_vgg_conv3x3_relu, (x + 48, o, o, x, 2, 2, 4, 4, null)),
        # max-pool
        (ARG, L.vst_vgg_maxpool2, (null, o, 2, 2, 4, null)), (ARG, L.vst_vgg_maxpool2, (x, null, 2, 2, 4, null)),
        (ARG, L.vst_vgg_maxpool2, (x4, o, 2, 2, 4, null)), (ARG, L.vst_vgg_maxpool2, (x, o + 8, 2, 2, 4, null)),
        (ARG, L.vst_vgg_maxpool2, (x, x, 2, 2, 4, null)), (ARG, L.vst_vgg_maxpool2, (x, x + 48, 2, 2, 4, null)),
        (SHAPE, L.vst_vgg_maxpool2, (x, o, 0, 2, 4, null)), (SHAPE, L.vst_vgg_maxpool2, (x, o, 2, 2, 6, null)),
        (SHAPE, L.vst_vgg_maxpool2, (x, o, 2, 2, 0, null)), (SHAPE, L.vst_vgg_maxpool2, (x, o, 4097, 4096, 4, null)),
        (SHAPE, L.vst_vgg_maxpool2, (x, o, 4096, 4096, 128, null)),
        # mean / std
        (ARG, L.vst_vgg_mean_std_workspace_bytes, (4, 4, null)), (SHAPE, L.vst_vgg_mean_std_workspace_bytes, (1, 4, C.byref(n))),
        (SHAPE, L.vst_vgg_mean_std_workspace_bytes, (4, 0, C.byref(n))), (SHAPE, L.vst_vgg_mean_std_workspace_bytes, (1 << 30, 2, C.byref(n))),
        (ARG, L.vst_vgg_mean_std, (null, 4, 4, 1e-5, o, ws, 1024, null)), (ARG, L.vst_vgg_mean_std, (x + 2, 4, 4, 1e-5, o, ws, 1024, null)),
        (ARG, L.vst_vgg_mean_std, (x, 4, 4, 1e-5, null, ws, 1024, null)), (ARG, L.vst_vgg_mean_std, (x, 4, 4, 1e-5, o + 4, ws, 1024, null)),
        (ARG, L.vst_vgg_mean_std, (x, 4, 4, -1.0, o, ws, 1024, null)), (ARG, L.vst_vgg_mean_std, (x, 4, 4, float("nan"), o, ws, 1024, null)),
        (SHAPE, L.vst_vgg_mean_std, (x, 1, 4, 1e-5, o, ws, 1024, null)), (SHAPE, L.vst_vgg_mean_std, (x, 4, 0, 1e-5, o, ws, 1024, null)),
        (WORKSPACE, L.vst_vgg_mean_std, (x, 4, 4, 1e-5, o, null, 1024, null)), (WORKSPACE, L.vst_vgg_mean_std, (x, 4, 4, 1e-5, o, ws + 4, 1024, null)),
        (WORKSPACE, L.vst_vgg_mean_std, (x, 4, 4, 1e-5, o, ws, 31, null)),
        # MSE and the loss
        (ARG, L.vst_vgg_mse_f64, (null, x, 4, o, ws, null)), (ARG, L.vst_vgg_mse_f64, (x, null, 4, o, ws, null)),
        (ARG, L.vst_vgg_mse_f64, (x + 2, x, 4, o, ws, null)), (ARG, L.vst_vgg_mse_f64, (x, x, 4, null, ws, null)),
        (ARG, L.vst_vgg_mse_f64, (x, x, 4, o + 4, ws, null)), (SHAPE, L.vst_vgg_mse_f64, (x, x, 0, o, ws, null)),
        (SHAPE, L.vst_vgg_mse_f64, (x, x, (1 << 30) + 1, o, ws, null)), (WORKSPACE, L.vst_vgg_mse_f64, (x, x, 4, o, null, null)),
        (WORKSPACE, L.vst_vgg_mse_f64, (x, x, 4, o, ws + 4, null)),
        (ARG, L.vst_vgg_style_loss, (null, x, o, null)), (ARG, L.vst_vgg_style_loss, (x, null, o, null)),
        (ARG, L.vst_vgg_style_loss, (x, x, null, null)), (ARG, L.vst_vgg_style_loss, (x4, x, o, null)),
        (ARG, L.vst_vgg_style_loss, (x, x, o + 4, null)),
        # plan
        (ARG, L.vst_vgg_create, (null,)), (ARG, L.vst_vgg_load_tensor, (null, b"0.weight", x, 9)), (ARG, L.vst_vgg_destroy, (null,)),
        (ARG, L.vst_vgg_workspace_bytes, (9, 9, null)), (SHAPE, L.vst_vgg_workspace_bytes, (8, 8, C.byref(n))),
        (SHAPE, L.vst_vgg_workspace_bytes, (8, 64, C.byref(n))), (SHAPE, L.vst_vgg_workspace_bytes, (64, 8, C.byref(n))),
        (SHAPE, L.vst_vgg_workspace_bytes, (4097, 4096, C.byref(n))),
    ]
    big = 1 << 40
    for f in (L.vst_vgg_features_u8, L.vst_vgg_features_f32):
        calls += [
            (ARG, f, (null, null, 9, 9, o, null, ws, big, null)), (ARG, f, (null, x, 9, 9, null, null, ws, big, null)),
            (ARG, f, (null, x, 9, 9, o + 4, null, ws, big, null)), (ARG, f, (null, x, 9, 9, o, x4, ws, big, null)),
            (SHAPE, f, (null, x, 8, 8, o, null, ws, big, null)), (SHAPE, f, (null, x, 8, 9, o, null, ws, big, null)),
            (SHAPE, f, (null, x, 9, 8, o, null, ws, big, null)), (SHAPE, f, (null, x, 4097, 4096, o, null, ws, big, null)),
            (WORKSPACE, f, (null, x, 9, 9, o, null, null, big, null)), (WORKSPACE, f, (null, x, 9, 9, o, null, ws + 4, big, null)),
            (WORKSPACE, f, (null, x, 9, 9, o, null, ws, 64, null)),
            (ARG, f, (null, x, 9, 9, o, null, ws, big, null)),          # everything fits but there is no plan
        ]
    calls.append((ARG, L.vst_vgg_features_f32, (null, x + 2, 9, 9, o, null, ws, big, null)))
    for i, (want, f, args) in enumerate(calls):
        assert f(*args) == want, (i, f.__name__, args)


def test_workspace_bytes():
    from vstnet_amd import vgg
    assert vgg.level_sizes(9, 9) == [(9, 9), (5, 5), (3, 3), (2, 2)]
    assert vgg.level_sizes(1080, 1920)[3] == (135, 240)
    small, hd = vgg.workspace_bytes(9, 9), vgg.workspace_bytes(1080, 1920)
    assert small >= 4 * (81 * 4 + 2 * 81 * 64)
    # the input map, two maps of H W 64 floats and at most 4 MiB of partial sums
    assert 4 * 1080 * 1920 * (4 + 128) <= hd <= 4 * 1080 * 1920 * (4 + 128) + (4 << 20) + 4096
    with pytest.raises(_lib.VstError):
        vgg.workspace_bytes(8, 8)


# ---------------------------------------------------------------------------------------------------------- drop-in
def test_models_vgg_signatures():
    """the reference's import path: the names and the signatures are the contract"""
    from models import VGG
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(VGG.calc_mean_std) == [("feat", E), ("eps", 1e-5)]
    assert params(VGG.VGG19.__init__)[:2] == [("self", E), ("checkpoint", "synthetic")]
    assert params(VGG.VGG19.encode_with_intermediate) == [("self", E), ("x", E), ("n_layer", 4)]
    assert params(VGG.VGG19.encode) == [("self", E), ("x", E), ("n_layer", 4)]
    assert params(VGG.VGG19.calc_content_loss) == [("self", E), ("input", E), ("target", E)]
    assert params(VGG.VGG19.calc_style_loss) == [("self", E), ("input", E), ("target", E)]
    assert params(VGG.VGG19.forward) == [("self", E), ("content_images", E), ("style_images", E), ("stylized_images", E),
                                         ("n_layer", 4), ("content_weight", 0)]
    assert issubclass(VGG.VGG19, torch.nn.Module)


def test_host_tensors_are_refused():
    """no CPU fallback: a tensor off the GPU is an error, never a quiet torch computation"""
    from vstnet_amd import vgg
    with pytest.raises(ValueError):
        vgg.mean_std(torch.zeros((4, 4)))
    with pytest.raises(ValueError):
        vgg.maxpool2(torch.zeros((4, 4)), 2, 2)
    with pytest.raises(ValueError):
        vgg.conv3x3_relu(torch.zeros((4, 4)), torch.zeros((4, 36)), torch.zeros(4), 2, 2)
    with pytest.raises(ValueError):
        vgg.input_map(torch.zeros((2, 2, 3), dtype=torch.uint8), torch.zeros(9), torch.zeros(3))


def test_reflect_col_is_the_conv():
    """the column matrix of the explicit route against F.conv2d on the reflect-padded map, in fp64"""
    g = torch.Generator().manual_seed(5)
    for h, w, cin, cout in ((2, 2, 4, 3), (3, 5, 8, 5), (5, 4, 4, 2)):
        x = torch.randn((h * w, cin), generator=g, dtype=torch.float64)
        wt = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64)
        want = torch.nn.functional.conv2d(torch.nn.functional.pad(x.t().reshape(1, cin, h, w), (1, 1, 1, 1), mode="reflect"), wt)
        got = R.reflect_col(x, h, w) @ R.pack_weight(wt).t()
        assert torch.allclose(got, R.tokens(want), rtol=1e-13, atol=1e-13)
    w3 = torch.randn((2, 3, 3, 3), generator=g)
    p = R.pack_weight(w3)
    assert p.shape == (2, 36) and float(p.reshape(2, 9, 4)[:, :, 3].abs().max()) == 0 and torch.equal(p.reshape(2, 3, 3, 4)[:, 1, 2, :3], w3[:, :, 1, 2])


# ----------------------------------------------------------------------------------------------------------- scripts
def test_csv_helpers(tmp_path):
    from vstnet_amd import style_files as S
    rows = {2: (0.1, 0.25), 0: (1.0 / 3.0, 2e-3), 1: (7.5e-2, 1e-9)}
    path = S.write_csv(str(tmp_path / S.CSV_NAME), rows)
    lines = open(path).read().splitlines()
    assert [ln.split(",")[0] for ln in lines] == ["0", "1", "2"] and lines[0] == "0,%r,%r" % (1.0 / 3.0, 2e-3)
    assert S.read_csv(path) == rows
    assert S.write_csv(str(tmp_path / "again.csv"), S.read_csv(path)) and open(tmp_path / "again.csv", "rb").read() == open(path, "rb").read()
    # the shards' parts, in any order, give the file one process writes; loss_s alone has two cells
    p0 = S.write_csv(str(tmp_path / S.part_name(0)), {0: rows[0], 1: rows[1]})
    p1 = S.write_csv(str(tmp_path / S.part_name(1)), {2: rows[2]})
    joined = S.join_parts([p1, p0], str(tmp_path / "joined.csv"), 3)
    assert open(joined, "rb").read() == open(path, "rb").read()
    with pytest.raises(ValueError, match="frame 2"):
        S.join_parts([p0], str(tmp_path / "x.csv"), 3)
    with pytest.raises(ValueError, match="more than one"):
        S.join_parts([p0, p0], str(tmp_path / "x.csv"))
    with pytest.raises(FileNotFoundError):
        S.join_parts([p0, str(tmp_path / S.part_name(7))], str(tmp_path / "x.csv"))
    (tmp_path / "bad.csv").write_text("0,1,2,3\n")
    with pytest.raises(ValueError, match="line 1"):
        S.read_csv(str(tmp_path / "bad.csv"))
    assert S.read_csv(S.write_csv(str(tmp_path / "one.csv"), {0: (0.5,)})) == {0: (0.5,)}
    text = S.summary(rows)
    assert "3 frames" in text and "loss_s mean %.6e max %.6e (frame 0)" % ((0.1 + 1 / 3 + 7.5e-2) / 3, 1 / 3) in text
    assert "loss_c mean" in text and "(frame 2)" in text and "loss_c" not in S.summary({0: (0.5,)})
    assert S.summary({}) == "style loss: no frames"


CHILD = r"""
import contextlib, io, json, os, sys
sys.path.insert(0, sys.argv[1])
tmp = sys.argv[2]
import image_transfer, video_transfer
out = {}
def run(name, main, argv):
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            main(argv)
        code = 0
    except SystemExit as e:
        code = e.code
    out[name] = [code, err.getvalue()[-600:]]
vid = ["--video", tmp + "/frames", "--style", tmp + "/s.png", "--max_size", "32", "--out_dir", tmp + "/o"]
img = ["--content", tmp + "/frames/000.png", "--style", tmp + "/s.png", "--max_size", "32", "--out_dir", tmp + "/o", "--synthetic_weights"]
for name, main, base in (("video", video_transfer.main, vid), ("image", image_transfer.main, img)):
    run(name + "_neither", main, base + ["--style_loss"])
    run(name + "_both", main, base + ["--style_loss", "--synthetic_vgg_weights", "--vgg_ckpoint", tmp + "/vgg.pth"])
    run(name + "_content_alone", main, base + ["--content_loss"])
    run(name + "_weights_alone", main, base + ["--synthetic_vgg_weights"])
run("video_deep", video_transfer.main, vid + ["--style_loss", "--synthetic_vgg_weights", "--out_pix_fmt", "yuv420p10le"])
run("video_stub", video_transfer.main, vid + ["--style_loss", "--synthetic_vgg_weights", "--stub_stylise"])
run("video_small_style", video_transfer.main, vid[:2] + ["--style", tmp + "/tiny.png"] + vid[4:] + ["--style_loss", "--synthetic_vgg_weights"])
run("image_small_style", image_transfer.main, img[:2] + ["--style", tmp + "/tiny.png"] + img[4:] + ["--style_loss", "--synthetic_vgg_weights"])
run("image_tiled", image_transfer.main, ["--content", tmp + "/huge.png"] + img[2:4] + ["--max_size", "16384", "--out_dir", tmp + "/o",
                                         "--synthetic_weights", "--style_loss", "--synthetic_vgg_weights"])
run("image_guided", image_transfer.main, img + ["--style_loss", "--content_loss", "--synthetic_vgg_weights", "--upscale", "guided"])
out["written"] = os.path.exists(tmp + "/o")
print(json.dumps(out))
"""


def test_parser_errors_in_a_child_process(tmp_path):
    """exit status 2, the message on stderr, nothing written, no GPU touched: every case ends in parser.error"""
    import json
    import subprocess
    from PIL import Image
    (tmp_path / "frames").mkdir()
    for i in range(2):
        Image.fromarray(R.image_u8(40, 56, 60 + i)).save(tmp_path / "frames" / f"{i:03d}.png")
    Image.fromarray(R.image_u8(32, 40, 70)).save(tmp_path / "s.png")
    Image.new("1", (8200, 8200)).save(tmp_path / "huge.png")
    Image.fromarray(R.image_u8(8, 8, 71)).save(tmp_path / "tiny.png")
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got.pop("written") is False
    want = {"_neither": "exactly one of", "_both": "exactly one of", "_content_alone": "--content_loss goes with --style_loss",
            "_weights_alone": "go with --style_loss"}
    for script in ("video", "image"):
        for case, text in want.items():
            code, err = got.pop(script + case)
            assert code == 2 and text in err, (script, case, code, err)
    for case, text in (("video_deep", "high-bit-depth output"), ("video_stub", "--stub_stylise"), ("image_tiled", "tiled route"), ("video_small_style", "at least 9x9"),
                       ("image_small_style", "at least 9x9"),
                       ("image_guided", "--upscale guided")):
        code, err = got.pop(case)
        assert code == 2 and text in err and ("style_loss" in err or "content_loss" in err), (case, code, err)
    assert not got
