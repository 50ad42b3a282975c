"""--seg_window on the host: the window's weights, the warm-up range of a shard, the logit ring's size against a simulation of
the frame loop's schedule, the parser errors, the flicker share, and the new entry point in the header and the built library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_weights():
    from vstnet_amd.segformer import window_weights
    for n in range(1, 9):
        for decay in (1.0, 0.5, 0.9, 0.01):
            w = window_weights(n, decay)
            assert w.dtype == np.float32 and w.shape == (n,)
            assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-7
            assert all(w[k] >= w[k + 1] for k in range(n - 1)) and w[0] > 0          # by age: the current frame first
            for k in range(1, n):
                assert float(w[k]) / float(w[0]) == pytest.approx(decay ** k, rel=1e-6)      # (two fp32 roundings: 1.2e-7)
    assert np.array_equal(window_weights(4), np.full(4, 0.25, np.float32))             # decay = 1: uniform
    assert np.array_equal(window_weights(1, 0.3), np.ones(1, np.float32))
    # fewer frames than the window: the frames that exist, renormalised
    full, part = window_weights(4, 0.5).astype(np.float64), window_weights(2, 0.5).astype(np.float64)
    assert np.allclose(part, full[:2] / full[:2].sum(), rtol=1e-6, atol=0)
    assert np.allclose(part, [2 / 3, 1 / 3], rtol=1e-6, atol=0)
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            window_weights(3, bad)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            window_weights(bad)


def test_warmup_range():
    from video_transfer import warmup_range
    assert warmup_range(0, 4) == ()
    assert warmup_range(2, 4) == (0, 1)
    assert warmup_range(10, 4) == (7, 8, 9)
    assert warmup_range(5, 1) == ()


@pytest.mark.parametrize("window", range(1, 9))
def test_ring_size_and_slot_reuse(window):
    """FramePipeline.run's schedule, restated: frame t is submitted, then - once depth - 1 newer frames are queued - frame
    t - (depth - 1) is retired.  Frame t writes slot t % R and reads the slots of frames t - 1 .. t - window + 1."""
    from vstnet_amd.pipeline import logit_ring_slots
    for depth in range(1, 7):
        slots = logit_ring_slots(window, depth)
        assert slots == window + depth
        holds, reader, retired = [None] * slots, [None] * slots, -1
        for t in range(50):
            j = t % slots
            assert reader[j] is None or reader[j] <= retired, (window, depth, t)      # a write never meets an unretired reader
            holds[j], reader[j] = t, None
            for age in range(1, min(window, t + 1)):
                k = (t - age) % slots
                assert holds[k] == t - age, (window, depth, t, age)                   # and a read finds the frame it wants
                reader[k] = t
            if t + 1 > depth - 1:
                retired = t - (depth - 1)


def test_parser_errors_and_defaults(capsys):
    import video_transfer as vt
    parser = vt.build_parser()
    base = ["--video", "clip", "--style", "s.png"]
    auto = ["--auto_seg", "--synthetic_seg_weights", "--no_seg_remap"]

    def check(argv):
        args = parser.parse_args(argv)
        vt.check_seg_args(parser, args)
        vt.check_window_args(parser, args)
        return args
    a = check(base)
    assert (a.seg_window, a.seg_decay) == (1, 1.0)
    a = check(base + auto + ["--seg_window", "8", "--seg_decay", "0.5"])
    assert (a.seg_window, a.seg_decay) == (8, 0.5)
    for bad in ("0", "9", "-1"):
        with pytest.raises(SystemExit) as e:
            check(base + auto + ["--seg_window", bad])
        assert e.value.code == 2 and "--seg_window must be in 1..8" in capsys.readouterr().err
    for bad in ("0", "1.5", "-0.1"):
        with pytest.raises(SystemExit) as e:
            check(base + auto + ["--seg_window", "3", "--seg_decay", bad])
        assert e.value.code == 2 and "--seg_decay must be in (0, 1]" in capsys.readouterr().err
    for extra in ([], ["--content_seg_dir", "maps", "--style_seg", "s_seg.png"]):
        with pytest.raises(SystemExit) as e:
            check(base + extra + ["--seg_window", "3"])
        assert e.value.code == 2 and "--auto_seg" in capsys.readouterr().err


def test_flicker_share():
    from video_transfer import FlickerMeter
    a = np.zeros((4, 5), np.uint8)
    b = a.copy()
    b[0, :] = 3                      # 5 of 20 pixels change
    c = b.copy()
    c[3, 0] = 7                      # 1 of 20
    m = FlickerMeter()
    assert m.share == 0.0 and m.pairs == 0
    for x in (a, b, c):
        m(x)
    assert m.pairs == 2 and m.share == pytest.approx((5 / 20 + 1 / 20) / 2, abs=1e-15)
    m(np.zeros((2, 2), np.uint8))    # another size starts over: no pair
    assert m.pairs == 2


@pytest.fixture(scope="module")
def lib():
    from vstnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_library_exports_the_mix_entry(lib):
    from vstnet_amd import _lib
    from vstnet_amd.segformer import MAX_WINDOW
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    assert re.search(r"\bint\s+vst_seg_mix_logits\s*\(", hdr) and "vst_seg_mix_logits" in _lib.EXPORTS
    assert hasattr(lib, "vst_seg_mix_logits") and lib.vst_version() >= 108
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT vst_seg_mix_logits\b", out)
    m = re.search(r"#define\s+VST_SEG_MIX_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == MAX_WINDOW == _lib.SEG_MIX_MAX == 8
    m = re.search(r"#define\s+VST_KERNEL_SEG_MIX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.KERNEL_SEG_MIX and _lib.MISC_KERNELS[_lib.KERNEL_SEG_MIX] == "seg_mix"


def test_mix_argument_errors_come_before_any_launch(lib):
    """No GPU here: every one of these returns before it touches the device."""
    vp = C.c_void_p
    ptrs, w = (vp * 8)(*[0x1000 * (k + 1) for k in range(8)]), (C.c_float * 8)(*[0.125] * 8)
    out = vp(0x100000)
    assert lib.vst_seg_mix_logits(None, w, 2, 300, out, None) == -1
    assert lib.vst_seg_mix_logits(ptrs, None, 2, 300, out, None) == -1
    assert lib.vst_seg_mix_logits(ptrs, w, 2, 300, None, None) == -1
    assert lib.vst_seg_mix_logits(ptrs, w, 2, 300, vp(0x100004), None) == -1            # out not 8-byte aligned
    assert lib.vst_seg_mix_logits((vp * 2)(0x1000, 0x2004), w, 2, 300, out, None) == -1   # an input not 8-byte aligned
    assert lib.vst_seg_mix_logits((vp * 2)(0x1000, 0), w, 2, 300, out, None) == -1        # a null input
    assert lib.vst_seg_mix_logits((vp * 2)(0x1000, 0x100000), w, 2, 300, out, None) == -1  # out is an input
    assert lib.vst_seg_mix_logits((vp * 2)(0x1000, 0x100000 + 1192), w, 2, 300, out, None) == -1   # out overlaps an input's end
    assert lib.vst_seg_mix_logits((vp * 2)(0x1000, 0x100000 - 1192), w, 2, 300, out, None) == -1
    for n in (0, 9, -1):
        assert lib.vst_seg_mix_logits(ptrs, w, n, 300, out, None) == -2
    for count in (0, 151, (1 << 20) * 150 + 2):
        assert lib.vst_seg_mix_logits(ptrs, w, 2, count, out, None) == -2
