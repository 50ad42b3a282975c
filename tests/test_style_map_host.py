"""Style maps ("Style maps"), the parts that need no GPU: the C ABI (header, bindings, version, argument
checks that come before any GPU call), bind_style_map's validation, the loaders' weight arithmetic, the scripts' flags and their
refusals, the identity the feature rests on (on the oracle) and the mutants of the fp32 restatement."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import cpu_ref
from vstnet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cwct_ops_ref as O                                               # noqa: E402
import style_map_ref as R                                              # noqa: E402

NEW_EXPORTS = ["vst_cwct_apply_code_mix", "vst_revnet_decode_mix", "vst_revnet_decode_mix_u8", "vst_cwct_mix_acc"]
E_ARG, E_SHAPE, E_MODE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_new_entry_points(lib):
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    assert lib.vst_version() >= 112
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert getattr(lib, name).restype is C.c_int
    # a _mix call is its _blend call plus K and the weight rows
    for blend, mix in (("vst_cwct_apply_code_blend", "vst_cwct_apply_code_mix"), ("vst_revnet_decode_blend", "vst_revnet_decode_mix"),
                       ("vst_revnet_decode_blend_u8", "vst_revnet_decode_mix_u8")):
        assert len(getattr(lib, mix).argtypes) == len(getattr(lib, blend).argtypes) + 2, mix
    assert "Style maps (version 112)" in hdr and "models/cWCT.py:206-262" in hdr


def test_new_calls_check_their_arguments_before_any_launch(lib):
    fake, odd = C.c_void_p(4096), C.c_void_p(4096 + 4)
    mix = lib.vst_cwct_apply_code_mix
    for K in (0, 1, 9):
        assert mix(fake, fake, 16, 16, 2, fake, K, fake, None, None) == E_ARG, K
    assert mix(None, fake, 16, 16, 2, fake, 2, fake, None, None) == E_ARG
    assert mix(fake, None, 16, 16, 2, fake, 2, fake, None, None) == E_ARG
    assert mix(fake, fake, 16, 16, 2, None, 2, fake, None, None) == E_ARG
    assert mix(fake, fake, 16, 16, 2, fake, 2, None, None, None) == E_ARG
    assert mix(odd, fake, 16, 16, 2, fake, 2, fake, None, None) == E_ARG               # code off the 16-byte grid
    assert mix(fake, odd, 16, 16, 2, fake, 2, fake, None, None) == E_ARG
    assert mix(fake, fake, 16, 16, 2, odd, 2, fake, None, None) == E_ARG
    assert mix(fake, fake, 16, 16, 2, fake, 2, C.c_void_p(4097), None, None) == E_ARG  # floats off the 4-byte grid
    assert mix(fake, fake, 16, 16, 2, fake, 2, fake, C.c_void_p(4098), None) == E_ARG
    assert mix(fake, fake, 16, 16, 1, fake, 3, fake, None, None) == E_MODE             # rows of 128: two styles only
    assert mix(fake, fake, 16, 16, 3, fake, 2, fake, None, None) == E_MODE
    assert mix(fake, fake, 16, 18, 2, fake, 2, fake, None, None) == E_SHAPE
    acc = lib.vst_cwct_mix_acc
    assert acc(None, fake, fake, 32, 64, 1, None) == E_ARG and acc(fake, None, fake, 32, 64, 1, None) == E_ARG
    assert acc(fake, fake, None, 32, 64, 1, None) == E_ARG and acc(fake, fake, C.c_void_p(4098), 32, 64, 1, None) == E_ARG
    for N, L in ((0, 64), (257, 64), (32, 0)):
        assert acc(fake, fake, fake, N, L, 0, None) == E_SHAPE, (N, L)
    for fn, tail in ((lib.vst_revnet_decode_mix, (1, 3, 16, 16, 2, 0, None)), (lib.vst_revnet_decode_mix_u8, (1, 16, 16, 2, 0, None))):
        net = _lib.NetWeights()
        assert fn(C.byref(net), fake, fake, 1, fake, None, fake, fake, *tail) == E_ARG
        assert fn(C.byref(net), fake, fake, 9, fake, None, fake, fake, *tail) == E_ARG
        assert fn(C.byref(net), fake, None, 2, fake, None, fake, fake, *tail) == E_ARG
        assert fn(C.byref(net), fake, fake, 2, None, None, fake, fake, *tail) == E_ARG
        assert fn(C.byref(net), fake, fake, 2, fake, None, None, fake, *tail) == E_ARG
        art = tail[:-3] + (1,) + tail[-2:]
        assert fn(C.byref(net), fake, fake, 3, fake, None, fake, fake, *art) == E_MODE


# ------------------------------------------------------------------------------------------------------------ bind_style_map
def test_bind_style_map_rejects_bad_maps():
    from models.cWCT import cWCT
    cw = cWCT(precision="bf16x3")
    shape = (1, 32, 16, 24)
    ok = np.full((2, 16, 24), 0.5, np.float32)
    for bad in (np.full((2, 16, 20), 0.5, np.float32), np.full((16, 24), 1.0, np.float32), np.full((2, 2, 16, 24), 0.5, np.float32),
                torch.full((2, 24, 16), 0.5), np.full((1, 2, 1, 16, 24), 0.5, np.float32)):
        with pytest.raises(ValueError, match="resolution"):
            cw.bind_style_map(bad, shape, "cuda")
    for K in (1, 9):                                                   # wrong K
        with pytest.raises(ValueError, match="2..8"):
            cw.bind_style_map(np.full((K, 16, 24), 1.0 / K, np.float32), shape, "cuda")
    m = ok.copy()
    m[0, 3, 5], m[1, 3, 5] = -0.25, 1.25                               # sums to 1, but negative
    with pytest.raises(ValueError, match=">= 0"):
        cw.bind_style_map(m, shape, "cuda")
    for v in (float("nan"), float("inf")):
        m = ok.copy()
        m[1, 2, 2] = v
        with pytest.raises(ValueError, match="finite"):
            cw.bind_style_map(torch.from_numpy(m)[None], shape, "cuda")
    for d in (1e-4, -1e-4):                                            # the sum: within 1e-5
        m = ok.copy()
        m[0, 7, 7] += d
        with pytest.raises(ValueError, match="sum to 1"):
            cw.bind_style_map(m, shape, "cuda")
    with pytest.raises(RuntimeError):                                  # a good map: only the device is missing
        cw.bind_style_map(ok, shape, "cpu")
    m = ok.copy()
    m[0, 7, 7] += 5e-6
    with pytest.raises(RuntimeError):
        cw.bind_style_map(m, shape, "cpu")
    assert cw.last_style_map is None
    assert "style_map" not in cWCT.ROUTES and "style_map" not in cWCT.INTERP_ROUTES     # a style map is not a route


def test_refusals_that_need_no_device():
    from vstnet_amd import tiled
    from vstnet_amd.code import PackedCode
    with pytest.raises(ValueError, match="style map"):
        tiled.stylize_tiled(None, None, np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), style_map=np.ones((2, 8, 8)))
    with pytest.raises(ValueError, match="style map"):
        tiled.stylize_whole(None, None, np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), style_map=np.ones((2, 8, 8)))
    # PackedCode.with_affines checks the weight rows like the strength rows
    z = PackedCode(torch.zeros(1, 32 * 8 * 8), 8, 8, None, None, 2)
    aff = torch.zeros(1, 2, 1056)
    assert z.with_affines(aff, None, mix=torch.zeros(1, 2, 64)).pending_mix is not None
    for bad in (torch.zeros(1, 2, 63), torch.zeros(1, 1, 64), torch.zeros(1, 9, 64), torch.zeros(2, 64), torch.zeros(1, 2, 64).double()):
        with pytest.raises(ValueError):
            z.with_affines(aff, None, mix=bad)
    with pytest.raises(ValueError):
        z.with_affines(torch.zeros(1, 3, 1056), None, mix=torch.zeros(1, 2, 64))
    za = PackedCode(torch.zeros(1, 32 * 8 * 8), 8, 8, None, None, 1)
    with pytest.raises(ValueError, match="two styles"):
        za.with_affines(torch.zeros(1, 3, 128 * 129), None, mix=torch.zeros(1, 3, 16))
    assert z.pending_mix is None and "mix of 2" in repr(z.with_affines(aff, None, mix=torch.zeros(1, 2, 64)))


# ------------------------------------------------------------------------------------------------------------ loaders
def _grey(path, h, w, fn):
    yy, xx = np.mgrid[0:h, 0:w]
    m = fn(yy, xx).astype(np.uint8)
    Image.fromarray(m).save(path)
    return m


def _rgb(path, h, w, seed):
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


def test_loader_weight_arithmetic(tmp_path):
    from image_transfer import load_style_map
    from utils.utils import style_map_weights
    ramp = _grey(tmp_path / "r.png", 24, 40, lambda y, x: (x * 255) // 39)
    w = load_style_map([str(tmp_path / "r.png")], (40, 24), "photorealistic")
    t = ramp.astype(np.float32) / np.float32(255)
    assert w.dtype == np.float32 and w.shape == (2, 24, 40)
    assert np.array_equal(w[1], t) and np.array_equal(w[0], np.float32(1) - t)
    assert np.all(w[0, :, 0] == 1) and np.all(w[1, :, 0] == 0) and np.all(w[0, :, -1] == 0) and np.all(w[1, :, -1] == 1)
    assert np.array_equal(w, R.loader_weights([ramp]))
    # resized like --strength_map: BILINEAR to the stylised size, BOX to the half-size grid for artistic codes
    big = load_style_map([str(tmp_path / "r.png")], (80, 48), "photorealistic")
    v = np.asarray(Image.fromarray(ramp).resize((80, 48), Image.BILINEAR))
    assert big.shape == (2, 48, 80) and np.array_equal(big, R.loader_weights([v]))
    art = load_style_map([str(tmp_path / "r.png")], (80, 48), "artistic")
    va = np.asarray(Image.fromarray(ramp).resize((80, 48), Image.BILINEAR).resize((40, 24), Image.BOX))
    assert art.shape == (2, 24, 40) and np.array_equal(art, R.loader_weights([va]))
    # K files: v_k / sum_j v_j, the sum in integers (three planes of 255 would overflow an 8-bit sum)
    planes = [_grey(tmp_path / f"p{k}.png", 24, 40, fn) for k, fn in enumerate(
        (lambda y, x: 255 - (x * 255) // 39, lambda y, x: (y * 255) // 23, lambda y, x: np.full_like(x, 255)))]
    w3 = load_style_map([str(tmp_path / f"p{k}.png") for k in range(3)], (40, 24), "photorealistic")
    tot = sum(p.astype(np.int64) for p in planes)
    assert tot.max() > 255 and w3.shape == (3, 24, 40)
    for k in range(3):
        assert np.array_equal(w3[k], planes[k].astype(np.float32) / tot.astype(np.float32))
    assert np.array_equal(w3, R.loader_weights(planes)) and float(np.abs(w3.sum(0) - 1).max()) <= 1e-6
    a3 = load_style_map([str(tmp_path / f"p{k}.png") for k in range(3)], (40, 24), "artistic")
    boxed = [np.asarray(Image.fromarray(p).resize((20, 12), Image.BOX)) for p in planes]
    assert a3.shape == (3, 12, 20) and np.array_equal(a3, R.loader_weights(boxed))
    # a pixel that no plane covers: named
    z0 = np.full((24, 40), 9, np.uint8)
    z0[5, 7] = 0
    with pytest.raises(ValueError, match=r"x = 7, y = 5"):
        style_map_weights([z0, z0.copy()])
    assert style_map_weights([z0]).shape == (2, 24, 40)                # (one plane: black is the first style, not an error)


def _inputs(tmp_path):
    _rgb(tmp_path / "c.png", 16, 24, 0)
    for k in range(3):
        _rgb(tmp_path / f"s{k}.png", 16, 16, 1 + k)
    _grey(tmp_path / "m.png", 16, 24, lambda y, x: (x * 255) // 23)
    hole = np.full((16, 24), 200, np.uint8)
    hole[3, 4] = 0
    Image.fromarray(hole).save(tmp_path / "h0.png")
    Image.fromarray(hole).save(tmp_path / "h1.png")
    Image.fromarray(np.zeros((16, 24), np.uint8)).save(tmp_path / "seg.png")
    (tmp_path / "clip").mkdir(exist_ok=True)
    (tmp_path / "segs").mkdir(exist_ok=True)
    for i in range(2):
        _rgb(tmp_path / "clip" / f"{i:03d}.png", 16, 24, 5 + i)
        Image.fromarray(np.zeros((16, 24), np.uint8)).save(tmp_path / "segs" / f"{i:03d}.png")


def _refusals(tmp):
    """(name, script, extra flags, what stderr must name): every argparse refusal of the flags"""
    s2, s3 = ["--styles", tmp + "/s0.png", tmp + "/s1.png"], ["--styles"] + [tmp + f"/s{k}.png" for k in range(3)]
    m, ms2 = ["--style_map", tmp + "/m.png"], ["--style_maps", tmp + "/m.png", tmp + "/m.png"]
    both = ("image", "video")
    cases = []
    for sc in both:
        cases += [
            (sc + "_one_style", sc, m, "--style_map"),
            (sc + "_three_styles_one_map", sc, s3 + m, "--style_map"),
            (sc + "_maps_count", sc, s3 + ms2, "--style_maps"),
            (sc + "_maps_one_style", sc, ["--style_maps", tmp + "/m.png"], "--style_maps"),
            (sc + "_both_flags", sc, s2 + m + ms2, "mutually exclusive"),
            (sc + "_alpha_s", sc, s2 + m + ["--alpha_s", "0.5", "0.5"], "--alpha_s"),
            (sc + "_missing", sc, s2 + ["--style_map", tmp + "/nope.png"], "no such file"),
            (sc + "_content_seg", sc, s2 + m + ["--content_seg", tmp + "/seg.png"], "masked"),
            (sc + "_style_segs", sc, s2 + m + ["--style_segs", tmp + "/seg.png", tmp + "/seg.png"], "masked"),
            (sc + "_style_seg", sc, s2 + m + ["--style_seg", tmp + "/seg.png"], "masked"),
            (sc + "_auto_seg", sc, s2 + m + ["--auto_seg", "--synthetic_seg_weights", "--no_seg_remap"], "auto_seg"),
            (sc + "_interpolate_labels", sc, s2 + m + ["--interpolate_labels"], "masked"),
            (sc + "_all_zero_pixel", sc, s2 + ["--style_maps", tmp + "/h0.png", tmp + "/h1.png"], "x = 4, y = 3"),
        ]
    cases += [("video_alpha_s_end", "video", s2 + m + ["--alpha_s_end", "0.2", "0.8"], "--alpha_s"),
              ("video_content_seg_dir", "video", s2 + m + ["--content_seg_dir", tmp + "/segs", "--style_seg", tmp + "/seg.png"], "masked"),
              ("video_gpus2", "video", s3 + m + ["--gpus", "2"], "--style_map")]
    return cases


CHILD = r"""
import json, sys
import torch
sys.path.insert(0, sys.argv[1])
tmp = sys.argv[2]
sys.path.insert(0, sys.argv[1] + "/tests")
import image_transfer, video_transfer
from test_style_map_host import _refusals
from vstnet_amd import tiled
codes = {}
def run(name, fn, argv):
    try:
        fn(argv)
        codes[name] = "returned"
    except SystemExit as e:
        codes[name] = e.code
img = ["--content", tmp + "/c.png", "--style", tmp + "/s0.png", "--synthetic_weights", "--out_dir", tmp + "/o"]
vid = ["--video", tmp + "/clip", "--style", tmp + "/s0.png", "--out_dir", tmp + "/ov", "--stub_stylise", "--frames_only"]
for name, script, extra, _ in _refusals(tmp):
    sys.stderr.write("CASE " + name + "\n")
    run(name, image_transfer.main if script == "image" else video_transfer.main, (img if script == "image" else vid) + extra)
sys.stderr.write("CASE video_stub\n")
run("video_stub", video_transfer.main, vid + ["--styles", tmp + "/s0.png", tmp + "/s1.png", "--style_map", tmp + "/m.png"])
tiled.max_frame_pixels = lambda: 100            # (the real guard is 2^26 pixels)
sys.stderr.write("CASE image_tiled\n")
run("image_tiled", image_transfer.main, img + ["--styles", tmp + "/s0.png", tmp + "/s1.png", "--style_map", tmp + "/m.png"])
print("RESULT " + json.dumps({"codes": codes, "gpu_initialised": torch.cuda.is_initialized()}))
"""


def test_every_refusal_is_an_argparse_error_before_any_gpu_work(tmp_path):
    """both scripts in a FRESH interpreter, which must end without having initialised the GPU: every refusal exits with status 2
    and names its flag; the stub rehearsal of the video script runs through with the flag"""
    _inputs(tmp_path)
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["gpu_initialised"] is False
    sections = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, _, text = chunk.partition("\n")
        sections[name] = text
    for name, _, _, needle in _refusals(str(tmp_path)):
        assert res["codes"][name] == 2, (name, res["codes"][name], sections.get(name, "")[-500:])
        assert needle in sections[name], (name, needle, sections[name][-500:])
    assert res["codes"]["video_stub"] == "returned"
    assert res["codes"]["image_tiled"] == 2 and "tiled" in sections["image_tiled"]


def test_both_parsers_accept_the_flags():
    import image_transfer
    import video_transfer
    for mod in (image_transfer, video_transfer):
        p = mod.build_parser()
        a = p.parse_args([])
        assert a.style_map is None and a.style_maps is None
        assert p.parse_args(["--style_map", "m.png"]).style_map == "m.png"
        assert p.parse_args(["--style_maps", "a.png", "b.png", "c.png"]).style_maps == ["a.png", "b.png", "c.png"]


# ------------------------------------------------------------------------------------------------------------ the identity
@pytest.mark.parametrize("N", [32, 128])
def test_interpolation_is_the_weighted_sum_of_single_style_transfers(N):
    """cpu_ref: interpolation(c, [s_k], [a_k], alpha_c) = sum_k a_k interpolation(c, [s_k], [1], alpha_c) for weights that sum
    to 1.  Tolerance: four times the relative-L2 figures DESIGN.md section 5 records for the strength identity, 3.8e-7 (fp32)
    and 3.3e-8 (use_double, whose result is stored as fp32).  Measured here: N = 32: 6.8e-8 / 3.0e-8; N = 128: 7.4e-8 / 3.0e-8."""
    rng = np.random.default_rng(N)
    c = torch.from_numpy(rng.standard_normal((1, N, 24, 40)).astype(np.float32)) * 0.7 + 0.2
    ss = [torch.from_numpy(rng.standard_normal((1, N, 20, 36)).astype(np.float32)) * (1.2 - 0.2 * k) - 0.1 * k for k in range(3)]
    al = [0.5, 0.3, 0.2]
    for dbl, tol in ((False, 4 * 3.8e-7), (True, 4 * 3.3e-8)):
        ref = cpu_ref.interpolation(c, ss, al, 0.3, use_double=dbl).double()
        mix = sum(a * cpu_ref.interpolation(c, [s], [1.0], 0.3, use_double=dbl).double() for a, s in zip(al, ss))
        err = float((ref - mix).norm() / ref.norm())
        print(f"N={N} use_double={dbl}: rel-L2 {err:.3g}, bound {tol:.3g}")
        assert err <= tol, (N, dbl, err)


# ------------------------------------------------------------------------------------------------------------ the mutants
@pytest.mark.parametrize("N,K,rows", R.MIX_CASES, ids=lambda v: str(v))
def test_restatement_and_its_mutants(N, K, rows):
    """the fp32 restatement sits within the bound of the fp64 sum, and each mutant (weights of rows swapped between k = 0 and
    k = 1; t0_k added unweighted) exceeds 1.25 x FACTOR["apply"] in the GPU test's metric"""
    x, affs, w = R.mix_input(N, K, rows, seed=1)
    assert float(np.abs(w.sum(0) - 1).max()) <= 1e-6 and w.min() >= 0
    hot = (w == 1).any(axis=0)
    assert hot[8:8 + rows // 4].all() and hot[rows // 2 - 2: rows // 2 + 2].all()      # the one-hot runs, across the halves
    want, den = R.mix64(x, affs, w, N)
    e32 = O.apply_err(R.mix32(x, affs, w, N), want, den)
    assert e32 <= 16 * O.U, e32 / O.U
    for m in R.MUTANTS:
        r = O.ratio("apply", O.apply_err(R.mix32(x, affs, w, N, mut=(m,)), want, den), e32)
        print(f"N={N} K={K} rows={rows}: e32 {e32 / O.U:.3g} u; mutant {m}: {r:.3g} x max(e32, floor), needs > {1.25 * O.FACTOR['apply']}")
        assert r > 1.25 * O.FACTOR["apply"], (m, r)
