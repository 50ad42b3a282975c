"""CPU: style interpolation under masks - the composed oracle against the reference's fixture, the route table, argument
validation, the exports, and the scripts' flags (alpha sum check, the stderr line, cross-fade weights per global frame index)."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from vstnet_amd import _lib
from tests.masked_interp_ref import interpolation_seg_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["vst_label_plan_hists", "vst_cwct_factor_labels_mix", "vst_cwct_prefactor_labels"]
T = torch.from_numpy


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# ------------------------------------------------------------------------------------------- the composed oracle
@pytest.mark.parametrize("key,ac,dbl,tol", [("out_ac0.0", 0.0, False, 2e-5), ("out_ac0.3", 0.3, False, 2e-5),
                                            ("out_ac0.3_f64", 0.3, True, 1e-6)])
def test_composition_matches_the_reference_fixture(golden, key, ac, dbl, tol):
    """tolerances: those oracle/make_golden.py uses for `interpolation` (2e-5 fp32, 1e-6 fp64)"""
    g = golden("cwct_masked_interp")
    c, sa, sb = T(g["c"]), T(g["sa"]), T(g["sb"])
    got = interpolation_seg_ref(c, [sa, sb], list(g["alphas"]), ac, g["cm"], [g["sma"], g["smb"]], use_double=dbl)
    assert rel_max(got, T(g[key])) <= tol
    # label 2 is valid against style A only: its pixels keep the content bits; the other labels moved
    keep = T(g["cm"][0] == 2)
    assert int(keep.sum()) > 10 and int((g["sma"][0] == 2).sum()) > 10 and int((g["smb"][0] == 2).sum()) <= 10
    assert torch.equal(T(g[key])[0][:, keep], c[0][:, keep]) and torch.equal(got[0][:, keep], c[0][:, keep])
    assert not torch.equal(got[0][:, ~keep], c[0][:, ~keep])


def test_composition_all_labels_valid(golden):
    g = golden("cwct_masked_interp")
    c, sa = T(g["c"]), T(g["sa"])
    got = interpolation_seg_ref(c, [sa, sa.flip(3)], [0.6, 0.4], 0.3, g["cm"], [g["sma"], g["sma"][:, :, ::-1].copy()])
    assert rel_max(got, T(g["out_all_valid"])) <= 2e-5
    assert float((got - c).abs().min()) > 0 or float((got != c).float().mean()) > 0.99


def test_one_style_alpha_one_is_transfer_seg(golden):
    """the reduction the device routes must keep bit for bit, on the oracle: interpolation([s], [1.0], 0) == _transfer_seg"""
    from oracle import cpu_ref
    g = golden("cwct_masked_interp")
    c, sa = T(g["c"]), T(g["sa"])
    a = interpolation_seg_ref(c, [sa], [1.0], 0.0, g["cm"], [g["sma"]])
    b = cpu_ref.transfer_seg(c, sa, g["cm"], g["sma"])
    assert rel_max(a, b) <= 2e-5


# ------------------------------------------------------------------------------------------- routes, arguments, exports
def test_route_table_and_answers():
    from models.cWCT import cWCT
    assert set(cWCT.INTERP_ROUTES) == {"interp_masked_single_pass", "interp_masked_packed_rows", "interp_masked_per_label"}
    assert not set(cWCT.INTERP_ROUTES) & (set(cWCT.ROUTES) | set(cWCT.WIDTH_ROUTES))
    for N in (32, 64, 128):
        assert cWCT.interp_route(False, N) == "interp_masked_single_pass"
        assert cWCT.interp_route(False, N, use_double=True) == "interp_masked_per_label"
    assert cWCT.interp_route(True, 32, sp_steps=2, max_slots=8) == "interp_masked_packed_rows"
    assert cWCT.interp_route(True, 32, sp_steps=2, max_slots=9) == "interp_masked_single_pass"
    assert cWCT.interp_route(True, 32, sp_steps=2, max_slots=0) == "interp_masked_single_pass"
    assert cWCT.interp_route(True, 128, sp_steps=1, max_slots=4) == "interp_masked_single_pass"
    for N in (16, 24, 100, 256):
        assert cWCT.interp_route(False, N) == "interp_masked_per_label"
    with pytest.raises(NotImplementedError):
        cWCT.interp_route(False, 257)


def test_argument_errors_come_before_any_device_work():
    """ValueError / AssertionError as `interpolation` raises today; nothing here needs a GPU"""
    from models.cWCT import cWCT
    cw = cWCT(precision="fp32")
    c = torch.zeros(1, 32, 8, 8)
    m = np.zeros((1, 8, 8), np.uint8)
    with pytest.raises(AssertionError):
        cw.interpolation(c, [c, c], [1.0])
    with pytest.raises(AssertionError):
        cw.interpolation(c, [c, c], [1.0], 0.0, m, [m, m])
    with pytest.raises(ValueError, match="at most 8"):
        cw.interpolation(c, [c] * 9, [1 / 9] * 9)
    with pytest.raises(ValueError, match="at most 8"):
        cw.interpolation(c, [c] * 9, [1 / 9] * 9, 0.0, m, [m] * 9)
    with pytest.raises(ValueError, match="one style label map per style"):
        cw.interpolation(c, [c, c], [0.5, 0.5], 0.0, m, [m])
    with pytest.raises(ValueError, match="cmask and smask_list"):
        cw.interpolation(c, [c], [1.0], 0.0, m, None)
    with pytest.raises(ValueError):
        cw.check_mix(0, [])
    cw.check_mix(8, [0.125] * 8, 8)


def test_header_and_exports(lib):
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    built = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_EXPORTS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in _lib.EXPORTS and name in built and hasattr(lib, name), name
    assert "cWCT.py:206-262" in hdr
    assert lib.vst_version() >= 105 and _lib.MAX_STYLES == 8


def test_new_calls_validate_arguments_before_any_launch(lib):
    import ctypes as C
    p, z = C.c_void_p(64), C.c_void_p(0)
    one = (C.c_void_p * 1)(64)
    nine = (C.c_void_p * 9)(*[64] * 9)
    hole = (C.c_void_p * 2)(64, 0)
    al = (C.c_float * 9)(*[1.0] * 9)
    E_ARG, E_SHAPE = -1, -2
    assert lib.vst_label_plan_hists(z, z, one, 1, 8, p, z, z) == E_ARG
    assert lib.vst_label_plan_hists(p, z, nine, 9, 8, p, z, z) == E_ARG and lib.vst_label_plan_hists(p, z, one, 0, 8, p, z, z) == E_ARG
    assert lib.vst_label_plan_hists(p, z, hole, 2, 8, p, z, z) == E_ARG
    assert lib.vst_label_plan_hists(p, z, one, 1, 0, p, z, z) == E_SHAPE and lib.vst_label_plan_hists(p, z, one, 1, 33, p, z, z) == E_SHAPE
    assert lib.vst_cwct_factor_labels_mix(p, nine, None, al, 9, 0.0, p, 8, 2e-5, 32, p, p, z) == E_ARG
    assert lib.vst_cwct_factor_labels_mix(p, hole, None, al, 2, 0.0, p, 8, 2e-5, 32, p, p, z) == E_ARG
    assert lib.vst_cwct_factor_labels_mix(p, one, None, al, 1, 0.0, z, 8, 2e-5, 32, p, p, z) == E_ARG
    assert lib.vst_cwct_factor_labels_mix(p, one, None, al, 1, 0.0, p, 8, 2e-5, 16, p, p, z) == E_SHAPE
    assert lib.vst_cwct_prefactor_labels(z, p, 8, 32, 2e-5, p, p, z) == E_ARG
    assert lib.vst_cwct_prefactor_labels(p, p, 8, 48, 2e-5, p, p, z) == E_SHAPE


# ------------------------------------------------------------------------------------------- the scripts
def _parse(mod, argv):
    args = mod.build_parser().parse_args(argv)
    err = io.StringIO()
    from image_transfer import check_mix_args
    return args, check_mix_args(args, err), err.getvalue()


def test_image_flags():
    import image_transfer as it
    args, per_label, err = _parse(it, ["--styles", "a.png", "b.png", "c.png"])
    assert args.alpha_s == [1 / 3] * 3 and args.style == "a.png" and not per_label and err == ""
    args, per_label, err = _parse(it, ["--style", "a.png", "--content_seg", "c.png", "--style_seg", "s.png", "--alpha_c", "0.3"])
    assert not per_label and err.count("\n") == 1 and "alpha_c is ignored" in err          # the reference's behaviour, said once
    args, per_label, err = _parse(it, ["--style", "a.png", "--content_seg", "c.png", "--style_seg", "s.png", "--alpha_c", "0.3",
                                       "--interpolate_labels"])
    assert per_label and err == "" and args.style_segs == ["s.png"]
    args, per_label, err = _parse(it, ["--styles", "a.png", "b.png", "--alpha_s", "0.25", "0.75", "--content_seg", "c.png",
                                       "--style_segs", "sa.png", "sb.png", "--interpolate_labels"])
    assert per_label and args.alpha_s == [0.25, 0.75] and args.style_seg == "sa.png"
    for bad in (["--styles", "a", "b", "--alpha_s", "0.5", "0.6"],                  # sum
                ["--styles", "a", "b", "--alpha_s", "0.5", "0.5", "0.0"],           # length
                ["--styles", "a", "b", "--alpha_s", "0.5", "0.500002"],             # within 1e-6
                ["--styles"] + ["s"] * 9,
                ["--styles", "a", "b", "--content_seg", "c", "--style_segs", "sa"],
                ["--styles", "a", "b", "--content_seg", "c", "--style_segs", "sa", "sb"],       # needs --interpolate_labels
                ["--styles", "a", "b", "--content_seg", "c", "--style_seg", "sa", "--interpolate_labels"]):
        with pytest.raises(SystemExit):
            _parse(it, bad)
    _parse(it, ["--styles", "a", "b", "--alpha_s", "0.5", "0.5000005"])


def _clip(d, n):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (36, 52, 3), dtype=np.uint8)).save(os.path.join(d, "%03d.png" % i))


def test_cross_fade_weights_follow_the_global_frame_index(tmp_path):
    import video_transfer as vt
    _clip(tmp_path / "clip", 7)
    for n in "ab":
        Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(tmp_path / f"{n}.png")
    base = ["--video", str(tmp_path / "clip"), "--styles", str(tmp_path / "a.png"), str(tmp_path / "b.png"), "--alpha_s", "1", "0",
            "--alpha_s_end", "0.25", "0.75", "--stub_stylise", "--frames_only", "--max_size", "48"]
    vt.main(base + ["--out_dir", str(tmp_path / "o1"), "--shard", "0/1"])
    whole = dict(vt.LAST_RUN["weights"])
    assert sorted(whole) == list(range(7))
    assert whole[0] == [1.0, 0.0] and whole[6] == [0.25, 0.75]
    for i in range(7):
        t = i / 6
        assert whole[i] == [(1 - t) * 1.0 + t * 0.25, (1 - t) * 0.0 + t * 0.75]
        assert abs(sum(whole[i]) - 1) < 1e-12
    union = {}
    for k in range(3):
        vt.main(base + ["--out_dir", str(tmp_path / "o3"), "--shard", "%d/3" % k])
        assert not set(vt.LAST_RUN["weights"]) & set(union)
        union.update(vt.LAST_RUN["weights"])
    assert union == whole                                    # identical floats: a frame's mix does not depend on its shard
    assert sorted(os.listdir(tmp_path / "o3" / "clip_a")) == sorted(os.listdir(tmp_path / "o1" / "clip_a"))
    with pytest.raises(SystemExit):
        vt.main(base[:-3] + ["--alpha_s_end", "0.5", "0.6", "--stub_stylise", "--out_dir", str(tmp_path / "o4")])


def test_video_says_once_that_alpha_c_is_ignored_under_masks(tmp_path):
    _clip(tmp_path / "clip", 2)
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(tmp_path / "s.png")
    Image.fromarray(np.zeros((20, 20), np.uint8)).save(tmp_path / "m.png")
    cmd = [sys.executable, os.path.join(REPO, "video_transfer.py"), "--video", str(tmp_path / "clip"), "--style", str(tmp_path / "s.png"),
           "--content_seg", str(tmp_path / "m.png"), "--style_seg", str(tmp_path / "m.png"), "--alpha_c", "0.3", "--stub_stylise",
           "--frames_only", "--out_dir", str(tmp_path / "o"), "--max_size", "48"]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr.count("alpha_c is ignored") == 1
    p = subprocess.run(cmd + ["--interpolate_labels"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert p.returncode == 0 and "alpha_c is ignored" not in p.stderr


def test_tiled_refuses_several_styles():
    from vstnet_amd import tiled
    img = np.zeros((8, 8, 3), np.uint8)
    for fn in (tiled.stylize_whole, tiled.stylize_tiled):
        with pytest.raises(ValueError, match="several styles in tiled mode are out of scope"):
            fn(None, None, img, [img, img], interpolate_labels=True)
