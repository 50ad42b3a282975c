"""Strength maps, the parts that need no GPU: the C ABI (header, bindings, version), the scripts' flag and
its errors, which come before any GPU work, the map loader and bind_strength's argument checks."""
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

from vstnet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["vst_map_to_code", "vst_cwct_apply_code_blend", "vst_cwct_apply_labels_code_blend", "vst_revnet_decode_blend",
               "vst_revnet_decode_blend_u8", "vst_revnet_decode_labels_blend", "vst_revnet_decode_labels_blend_u8", "vst_cwct_blend"]
E_ARG, E_SHAPE, E_MODE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declarations_equal_exports():
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    declared = set(re.findall(r"\b(vst_[a-z0-9_]+)\s*\(", hdr)) - {"vst_conv_weights", "vst_block_weights", "vst_net_weights"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name


def test_library_has_the_new_entry_points(lib):
    assert lib.vst_version() >= 109
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
    # each _blend call is its plain call plus one pointer
    for plain in ("vst_cwct_apply_code", "vst_cwct_apply_labels_code", "vst_revnet_decode", "vst_revnet_decode_u8",
                  "vst_revnet_decode_labels", "vst_revnet_decode_labels_u8"):
        blend = plain.replace("_u8", "") + "_blend" + ("_u8" if plain.endswith("_u8") else "")
        assert len(getattr(lib, blend).argtypes) == len(getattr(lib, plain).argtypes) + 1, blend


def test_new_calls_check_their_arguments_before_any_launch(lib):
    fake = C.c_void_p(4096)
    assert lib.vst_map_to_code(None, fake, 16, 16, 2, None) == E_ARG
    assert lib.vst_map_to_code(fake, fake, 16, 18, 2, None) == E_SHAPE
    assert lib.vst_map_to_code(fake, fake, 16, 16, 3, None) == E_MODE
    assert lib.vst_cwct_blend(fake, fake, None, fake, 32, 64, None) == E_ARG
    assert lib.vst_cwct_blend(fake, fake, fake, fake, 0, 64, None) == E_SHAPE
    assert lib.vst_cwct_blend(fake, fake, fake, fake, 257, 64, None) == E_SHAPE
    assert lib.vst_cwct_blend(fake, fake, fake, fake, 32, 0, None) == E_SHAPE
    assert lib.vst_cwct_apply_code_blend(fake, fake, 16, 16, 2, None, fake, None) == E_ARG
    assert lib.vst_cwct_apply_code_blend(fake, fake, 16, 18, 2, fake, fake, None) == E_SHAPE
    assert lib.vst_cwct_apply_labels_code_blend(fake, fake, 16, 16, fake, fake, fake, 9, fake, None) == E_SHAPE
    assert lib.vst_cwct_apply_labels_code_blend(fake, fake, 16, 16, fake, None, fake, 8, fake, None) == E_ARG


def _grey(path, h, w, value=None):
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx * 255) // max(1, w - 1)).astype(np.uint8) if value is None else np.full((h, w), value, np.uint8)
    Image.fromarray(m).save(path)
    return m


def _rgb(path, h, w, seed):
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


def test_both_parsers_accept_the_flag():
    import image_transfer
    import video_transfer
    for mod in (image_transfer, video_transfer):
        p = mod.build_parser()
        assert p.parse_args([]).strength_map is None
        assert p.parse_args(["--strength_map", "m.png"]).strength_map == "m.png"


def test_missing_file_is_an_error(tmp_path, capsys):
    import image_transfer
    import video_transfer
    _rgb(tmp_path / "c.png", 16, 24, 0)
    _rgb(tmp_path / "s.png", 16, 16, 1)
    with pytest.raises(SystemExit) as e:
        image_transfer.main(["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--synthetic_weights",
                             "--out_dir", str(tmp_path / "o"), "--strength_map", str(tmp_path / "nope.png")])
    assert e.value.code == 2 and "--strength_map" in capsys.readouterr().err
    fd = tmp_path / "clip"
    fd.mkdir()
    for i in range(2):
        _rgb(fd / f"{i:03d}.png", 16, 24, 2 + i)
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--out_dir", str(tmp_path / "ov"), "--stub_stylise",
            "--frames_only"]
    with pytest.raises(SystemExit) as e:
        video_transfer.main(base + ["--strength_map", str(tmp_path / "nope.png")])
    assert e.value.code == 2 and "--strength_map" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                    # the parent of --gpus N says so before it starts a child
        video_transfer.main(base + ["--strength_map", str(tmp_path / "nope.png"), "--gpus", "2"])
    assert e.value.code == 2 and "--strength_map" in capsys.readouterr().err
    # with the file there the stub rehearsal runs through (it stylises nothing and ignores the map)
    _grey(tmp_path / "m.png", 8, 8)
    out = video_transfer.main(base + ["--strength_map", str(tmp_path / "m.png")])
    assert sorted(os.listdir(out)) == ["00000.png", "00001.png"]


def test_tiled_route_is_an_error(tmp_path, capsys, monkeypatch):
    """An image past the whole-frame guard takes the tiled route, which has no strength maps.  (The guard is lowered for the
    test: the real one is 2^26 pixels.)"""
    import image_transfer
    from vstnet_amd import tiled
    _rgb(tmp_path / "c.png", 40, 48, 0)
    _rgb(tmp_path / "s.png", 16, 16, 1)
    _grey(tmp_path / "m.png", 8, 8)
    monkeypatch.setattr(tiled, "max_frame_pixels", lambda: 1000)
    with pytest.raises(SystemExit) as e:
        image_transfer.main(["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--synthetic_weights",
                             "--out_dir", str(tmp_path / "o"), "--strength_map", str(tmp_path / "m.png")])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--strength_map" in err and "tiled" in err


CHILD = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
tmp = sys.argv[2]
import image_transfer, video_transfer
from vstnet_amd import tiled
from models.cWCT import cWCT
codes = {}
def run(name, fn, argv):
    try:
        fn(argv)
        codes[name] = "returned"
    except SystemExit as e:
        codes[name] = e.code
img = ["--content", tmp + "/c.png", "--style", tmp + "/s.png", "--synthetic_weights", "--out_dir", tmp + "/o"]
vid = ["--video", tmp + "/clip", "--style", tmp + "/s.png", "--out_dir", tmp + "/ov", "--stub_stylise", "--frames_only"]
run("image_missing", image_transfer.main, img + ["--strength_map", tmp + "/nope.png"])
run("video_missing", video_transfer.main, vid + ["--strength_map", tmp + "/nope.png"])
run("video_missing_gpus2", video_transfer.main, vid + ["--strength_map", tmp + "/nope.png", "--gpus", "2"])
run("video_stub", video_transfer.main, vid + ["--strength_map", tmp + "/m.png"])
tiled.max_frame_pixels = lambda: 1000           # (the real guard is 2^26 pixels)
run("image_tiled", image_transfer.main, img + ["--strength_map", tmp + "/m.png"])
try:
    cWCT(precision="bf16x3").bind_strength(np.full((16, 24), 1.5, np.float32), (1, 32, 16, 24), "cuda")
    codes["bind"] = "returned"
except ValueError:
    codes["bind"] = "ValueError"
print("RESULT " + json.dumps({"codes": codes, "gpu_initialised": torch.cuda.is_initialized()}))
"""


def test_errors_come_before_any_gpu_work(tmp_path):
    """the error paths of both scripts and of bind_strength in a FRESH interpreter, which must end without having initialised
    the GPU (in this process an earlier test may have done that)"""
    _rgb(tmp_path / "c.png", 40, 48, 0)
    _rgb(tmp_path / "s.png", 16, 16, 1)
    _grey(tmp_path / "m.png", 8, 8)
    (tmp_path / "clip").mkdir()
    for i in range(2):
        _rgb(tmp_path / "clip" / f"{i:03d}.png", 16, 24, 2 + i)
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["codes"] == {"image_missing": 2, "video_missing": 2, "video_missing_gpus2": 2, "video_stub": "returned",
                            "image_tiled": 2, "bind": "ValueError"}
    assert res["gpu_initialised"] is False
    assert r.stderr.count("--strength_map") >= 4


def test_map_loader_sizes_and_values(tmp_path):
    from image_transfer import load_strength_map
    m = _grey(tmp_path / "m.png", 24, 40)
    s = load_strength_map(str(tmp_path / "m.png"), (40, 24), "photorealistic")
    assert s.dtype == np.float32 and s.shape == (24, 40)
    assert np.array_equal(s, m.astype(np.float32) / np.float32(255))           # same size: no resize, s = v / 255
    assert s.min() == 0.0 and s.max() == 1.0
    big = load_strength_map(str(tmp_path / "m.png"), (80, 48), "photorealistic")
    want = np.asarray(Image.fromarray(m).resize((80, 48), Image.BILINEAR), dtype=np.float32) / np.float32(255)
    assert big.shape == (48, 80) and np.array_equal(big, want)
    art = load_strength_map(str(tmp_path / "m.png"), (80, 48), "artistic")
    want = np.asarray(Image.fromarray(m).resize((80, 48), Image.BILINEAR).resize((40, 24), Image.BOX), dtype=np.float32)
    assert art.shape == (24, 40) and np.array_equal(art, want / np.float32(255))
    # a colour file is read as grey; white is exactly 1
    Image.fromarray(np.full((8, 8, 3), 255, np.uint8)).save(tmp_path / "w.png")
    assert np.all(load_strength_map(str(tmp_path / "w.png"), (16, 12), "photorealistic") == 1.0)


def test_bind_strength_rejects_bad_maps():
    from models.cWCT import cWCT
    cw = cWCT(precision="bf16x3")
    shape = (1, 32, 16, 24)
    ok = np.full((16, 24), 0.5, np.float32)
    for bad in (np.zeros((16, 20), np.float32), np.zeros((1, 16, 24), np.float32), np.zeros((2, 1, 16, 24), np.float32),
                torch.zeros(24, 16)):
        with pytest.raises(ValueError, match="resolution"):
            cw.bind_strength(bad, shape, "cuda")
    for v in (-0.01, 1.0001, float("nan")):
        m = ok.copy()
        m[3, 5] = v
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            cw.bind_strength(m, shape, "cuda")
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            cw.bind_strength(torch.from_numpy(m)[None, None], shape, "cuda")
    with pytest.raises(RuntimeError):
        cw.bind_strength(ok, shape, "cpu")
    assert cw.last_strength is None
