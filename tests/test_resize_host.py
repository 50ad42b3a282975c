"""Host side of the device resize (no GPU): the numpy restatement of Pillow's 8-bit bicubic resize is pinned against Pillow
itself, the library's coefficient tables against the restatement, the error codes, the size rule and the script's flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from tests import resize_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source w, h) -> (w, h): two 16:9 shrinks, two near-identity shrinks, two upscales
PIL_SHAPES = [((1920, 1080), (1280, 720)), ((3840, 2160), (1280, 720)), ((641, 363), (640, 360)), ((97, 55), (96, 52)),
              ((300, 200), (452, 300)), ((500, 333), (1280, 852))]
PAIRS = [(1920, 1280), (1080, 720), (3840, 1280), (641, 640), (363, 360), (200, 300), (7, 96)]


@pytest.mark.parametrize("src_wh,dst_wh", PIL_SHAPES)
def test_restatement_equals_pillow(src_wh, dst_wh):
    img = ref.frame(src_wh[1], src_wh[0], seed=src_wh[0])
    want = np.asarray(Image.fromarray(img).resize(dst_wh, Image.BICUBIC))
    got = ref.pil_resize(img, dst_wh)
    assert got.shape == want.shape
    assert int((got != want).sum()) == 0


def test_restatement_equals_pillow_smooth_and_same_size():
    img = ref.frame(363, 641, seed=3, smooth=True)
    assert np.array_equal(ref.pil_resize(img, (640, 360)), np.asarray(Image.fromarray(img).resize((640, 360), Image.BICUBIC)))
    assert np.array_equal(ref.pil_resize(img, (641, 363)), img)
    assert np.array_equal(ref.pil_resize(img, (641, 360)), np.asarray(Image.fromarray(img).resize((641, 360), Image.BICUBIC)))


def _lib():
    from vstnet_amd import _lib
    return _lib.lib()


def _tables(fn, in_size, out_size, dtype):
    ks = C.c_int(0)
    assert fn(in_size, out_size, C.byref(ks), None, None) == 0            # the query form
    bounds = np.full((out_size, 2), -7, np.int32)
    co = np.empty((out_size, ks.value), dtype)
    assert fn(in_size, out_size, C.byref(ks), C.c_void_p(bounds.ctypes.data), C.c_void_p(co.ctypes.data)) == 0
    return ks.value, bounds, co


@pytest.mark.parametrize("in_size,out_size", PAIRS)
def test_u8_tables_equal_the_restatement(in_size, out_size):
    ks, bounds, kk = _tables(_lib().vst_resize_coeffs_u8, in_size, out_size, np.int32)
    rks, rbounds, rkk = ref.pil_coeffs(in_size, out_size)
    assert ks == rks
    assert np.array_equal(bounds, rbounds)
    assert np.array_equal(kk, rkk)
    assert np.abs(kk.astype(np.int64)).sum(1).max() * 255 < 2 ** 31 - 2 ** 21       # the int32 accumulator is enough


@pytest.mark.parametrize("in_size,out_size", PAIRS + [(720, 1080), (716, 719), (256, 100)])
def test_f32_weights_equal_the_float64_formula(in_size, out_size):
    ks, bounds, w = _tables(_lib().vst_resize_coeffs_f32, in_size, out_size, np.float32)
    rks, rbounds, rw = ref.aa_weights_f64(in_size, out_size)
    assert ks == rks and np.array_equal(bounds, rbounds)
    err = np.abs(w.astype(np.float64) - rw)
    assert (err <= 2.0 ** -23 * np.abs(rw)).all(), float(err.max())      # fp32 storage of the double-built weight
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 4 * 2.0 ** -24 * ks


# ------------------------------------------------------------------------------------------------ the float resize's reference
from tests import resize_f32_ref as F32   # noqa: E402

F32_IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in F32.CASES]


@pytest.mark.parametrize("i", range(len(F32.CASES)), ids=F32_IDS)
def test_f32_reference_against_interpolate_in_float64(i):
    """the same function: F.interpolate(bicubic, antialias=True) on the float64 image computes its weights in float64 too, so
    the two agree to float64 rounding (1e-12 is 2^-53 with four decimal digits to spare on sums of at most 65 taps)"""
    import torch
    import torch.nn.functional as TF
    x, ref, e = F32.case(i)
    want = TF.interpolate(torch.tensor(x).double(), size=F32.CASES[i][1], mode="bicubic", align_corners=False, antialias=True)
    dev = float(np.abs(want.numpy() - ref).max())
    print(f"{F32_IDS[i]}: reference against F.interpolate in float64, max deviation {dev:.3e}; median E {np.median(e):.2e}")
    assert ref.shape == tuple(want.shape) and dev <= 1e-12


@pytest.mark.parametrize("i", range(len(F32.CASES)), ids=F32_IDS)
def test_f32_emulation_is_under_the_bound(i):
    """the kernels in numpy float32 (the library's own tables, one fma per tap) under E, the bytes under the byte rule; the
    share of the reference's values that the byte rule leaves open is at most 1 %"""
    x, ref, e = F32.case(i)
    (Hs, Ws), (Hd, Wd) = F32.CASES[i]
    for a, b in ((Ws, Wd), (Hs, Hd)):                           # the emulation's tables are the library's
        ks, bounds, w = _tables(_lib().vst_resize_coeffs_f32, a, b, np.float32)
        rks, rbounds, rw = F32.table(a, b)
        assert ks == rks and np.array_equal(bounds, rbounds) and np.array_equal(w, rw.astype(np.float32))
    out = F32.emulate(x, (Hd, Wd))
    ok, worst = F32.check_float(out, ref, e)
    okb, differ, maxd = F32.check_bytes(F32.quantise(out), ref, e)
    near = F32.to_bytes(ref, e)[3]
    free = (np.transpose(ref, (0, 2, 3, 1)) > 0) & (np.transpose(ref, (0, 2, 3, 1)) < 1)
    share = float((near & free).sum() / max(int(free.sum()), 1))
    print(f"{F32_IDS[i]}: emulation worst error / E {worst:.3f}, bytes that differ {differ} (max {maxd}), "
          f"255 ref within its bound of an integer {share:.2e} of the unclamped values")
    assert ok.all() and okb.all() and maxd <= 1
    assert share <= 1e-2
    if (Hs, Ws) == (1, 1):
        assert np.array_equal(out, np.broadcast_to(x, out.shape))           # one source pixel: the output is that pixel


def test_f32_planted_faults_fail():
    """each fault in the emulation fails the float comparison on some case; `rows` exactly on the cases with a horizontal pass
    whose planes do not hold a whole number of row groups; rounding fails the byte comparison"""
    for fault in ("rows", "first", "border"):
        caught = []
        for i in range(len(F32.CASES)):
            x, ref, e = F32.case(i)
            ok, worst = F32.check_float(F32.emulate(x, F32.CASES[i][1], fault), ref, e)
            if not ok.all():
                caught.append(i)
        print(f"planted fault {fault}: fails on {[F32_IDS[i] for i in caught]}")
        assert caught, fault
        if fault == "rows":
            assert caught == [i for i, ((hs, ws), (hd, wd)) in enumerate(F32.CASES) if ws != wd and hs % F32.H_ROWS]
            assert 1 in caught and 3 not in caught
    caught = []
    for i in range(len(F32.CASES)):
        x, ref, e = F32.case(i)
        if not F32.check_bytes(F32.quantise(F32.emulate(x, F32.CASES[i][1]), "round"), ref, e)[0].all():
            caught.append(i)
    print(f"planted fault rounding: fails on {[F32_IDS[i] for i in caught]}")
    assert len(caught) == len(F32.CASES) - 1 or len(caught) == len(F32.CASES)


def test_f32_reciprocal_filterscale_is_below_fp32_resolution():
    """`t * (1 / filterscale)` for `t / filterscale` (Pillow's form for the float resize's) was meant to be a planted fault
    that fails.  It cannot: both are evaluated in double, the arguments differ by an ulp of double, and the cubic is continuous,
    so the weights move by at most 1.4e-15 (measured here, largest over the cases' tables) and the fp32 emulation's output not
    by one bit.  No comparison at fp32 resolution can see it, on the host or on the card; this test pins that the
    substitution is harmless instead of claiming to catch it."""
    worst_w, worst_o = 0.0, 0.0
    for i, ((Hs, Ws), (Hd, Wd)) in enumerate(F32.CASES):
        for a, b in ((Ws, Wd), (Hs, Hd)):
            worst_w = max(worst_w, float(np.abs(F32.table(a, b, "reciprocal")[2] - F32.table(a, b)[2]).max()))
        x, ref, e = F32.case(i)
        d = np.abs(F32.emulate(x, (Hd, Wd), "reciprocal").astype(np.float64) - F32.emulate(x, (Hd, Wd)).astype(np.float64))
        worst_o = max(worst_o, float((d / e).max()))
        assert F32.check_float(F32.emulate(x, (Hd, Wd), "reciprocal"), ref, e)[0].all()
    print(f"reciprocal filterscale: weights move by at most {worst_w:.3e}, the emulation's output by at most {worst_o:.3e} E")
    assert worst_w <= 2.0 ** -48


def test_error_codes_without_a_gpu():
    L = _lib()
    ks = C.c_int(0)
    one = C.c_void_p(16)         # a non-null pointer nothing dereferences: every check comes before any launch
    assert L.vst_resize_coeffs_u8(100, 50, None, None, None) == -1
    assert L.vst_resize_coeffs_u8(0, 50, C.byref(ks), None, None) == -1
    assert L.vst_resize_coeffs_f32(100, -1, C.byref(ks), None, None) == -1
    assert L.vst_resize_coeffs_u8(17 * 50, 50, C.byref(ks), None, None) == -2
    assert L.vst_resize_coeffs_u8(16 * 50, 50, C.byref(ks), None, None) == 0 and ks.value == 65
    assert L.vst_resize_coeffs_f32(17 * 50, 50, C.byref(ks), None, None) == -2
    assert L.vst_resize_u8(None, 100, 100, one, 50, 50, one, one, None) == -1
    assert L.vst_resize_u8(one, 100, 100, None, 50, 50, one, one, None) == -1
    assert L.vst_resize_u8(one, 100, 100, one, 50, 50, None, one, None) == -1
    assert L.vst_resize_u8(one, 100, 100, one, 50, 0, one, one, None) == -1
    assert L.vst_resize_u8(one, 17 * 8, 100, one, 8, 50, one, one, None) == -2            # a 17x shrink, vertical
    assert L.vst_resize_u8(one, 100, 17 * 8, one, 50, 8, one, one, None) == -2            # ... horizontal
    assert L.vst_resize_u8(one, 8192, 8193, one, 4096, 4096, one, one, None) == -2        # source past VST_MAX_FRAME_PIXELS
    assert L.vst_resize_u8(one, 4096, 4096, one, 8193, 8192, one, one, None) == -2        # destination past it
    for fn in (L.vst_resize_f32, L.vst_resize_f32_to_u8):
        assert fn(None, 1, 100, 100, one, 50, 50, one, one, None) == -1
        assert fn(one, 1, 100, 100, None, 50, 50, one, one, None) == -1
        assert fn(one, 0, 100, 100, one, 50, 50, one, one, None) == -1
        assert fn(one, 1, 100, 100, one, 50, 50, one, None, None) == -1                   # a horizontal pass needs tmp
        assert fn(one, 1, 17 * 8, 100, one, 8, 50, one, one, None) == -2
        assert fn(one, 1, 8192, 8193, one, 4096, 4096, one, one, None) == -2


def test_size_rule_equals_img_resize():
    from utils.utils import img_resize
    from vstnet_amd.resize import img_resize_size, img_resize_steps, device_supported
    sizes = [(1920, 1080), (3840, 2160), (1283, 719), (1000, 562), (641, 363), (97, 55), (55, 97), (1279, 1281), (1281, 200),
             (333, 500), (129, 127), (4, 4), (1280, 1280), (2001, 1999)]
    for w, h in sizes:
        img = Image.new("RGB", (w, h))
        for max_size in (1280, 1279, 128, 97, 640):
            for ds in (4, None, 2):
                want = img_resize(img, max_size, down_scale=ds).size
                assert img_resize_size((w, h), max_size, ds) == want, (w, h, max_size, ds)
                steps = img_resize_steps((w, h), max_size, ds)
                assert len(steps) <= 2 and (not steps or steps[-1] == want)
    assert device_supported((1920, 1080), 1280, 4) and device_supported((3840, 2160), 1280, 4)
    assert not device_supported((3840, 2160), 128, 4)          # a 30x shrink: the host resizes
    assert not device_supported((1281, 3), 1280, 4)            # the floor to a multiple of 4 leaves no rows


def test_parser_accepts_resize():
    from video_transfer import build_parser
    p = build_parser()
    assert p.parse_args([]).resize == "host"
    assert p.parse_args(["--resize", "device"]).resize == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--resize", "gpu"])


def test_stub_run_with_device_resize_writes_writer_size_frames(tmp_path):
    rng = np.random.default_rng(1)
    os.makedirs(tmp_path / "clip")
    for i in range(3):
        Image.fromarray(rng.integers(0, 255, (54, 96, 3), dtype=np.uint8)).save(tmp_path / "clip" / ("%03d.png" % i))
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(tmp_path / "s.png")
    outs = {}
    for mode in ("host", "device"):
        p = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py"), "--video", str(tmp_path / "clip"), "--style",
                            str(tmp_path / "s.png"), "--out_dir", str(tmp_path / mode), "--stub_stylise", "--frames_only",
                            "--max_size", "64", "--resize", mode], capture_output=True, text=True, timeout=120, cwd=REPO)
        assert p.returncode == 0, p.stderr[-2000:]
        d = tmp_path / mode / "clip_s"
        outs[mode] = [np.asarray(Image.open(d / f)) for f in sorted(os.listdir(d))]
    from video_transfer import writer_size
    wsz = writer_size(Image.open(tmp_path / "clip" / "000.png"), 64)
    assert wsz == (64, 54)                                      # the writer-size quirk: the width shrinks, the height does not
    assert len(outs["device"]) == 3
    for a, b in zip(outs["host"], outs["device"]):
        assert b.shape == (wsz[1], wsz[0], 3)
        assert np.array_equal(a, b)                             # the stub rehearses the flag on the host resize
