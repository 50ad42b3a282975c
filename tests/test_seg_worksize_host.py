"""--seg_size / SegFormer.work_hw on the host: the size rule, the parser errors, the golden file's own invariants and the header."""
import os
import re
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"up4": (288, 416, 104, (72, 104)), "ragged": (283, 409, 101, (70, 101)), "chain": (144, 208, 104, (72, 104)),
         "same": (96, 136, 136, (96, 136))}


@pytest.mark.parametrize("case", sorted(CASES))
def test_work_hw_of_the_golden_cases(case):
    from vstnet_amd.segformer import SegFormer
    h, w, size, want = CASES[case]
    assert SegFormer.work_hw(h, w, size) == want


@pytest.mark.parametrize("hw, size, want", [
    ((720, 1280), 512, (288, 512)), ((720, 1280), 640, (360, 640)), ((720, 1280), 1024, (576, 1024)),
    ((1080, 1920), 512, (288, 512)), ((1080, 1920), 640, (360, 640)), ((1080, 1920), 1024, (576, 1024)),
    ((1280, 720), 512, (512, 288)),
    ((720, 1280), 1280, (720, 1280)), ((720, 1280), 4096, (720, 1280)), ((720, 1280), None, (720, 1280)),
    ((40, 4000), 400, (32, 400)),                  # the short edge is kept at the network's minimum
    ((101, 203), 100, (50, 100)),                  # 49.75 rounds half up
])
def test_work_hw_rule(hw, size, want):
    from vstnet_amd.segformer import SegFormer
    assert SegFormer.work_hw(hw[0], hw[1], size) == want


def test_work_hw_refuses_sizes_under_32():
    from vstnet_amd.segformer import SegFormer
    with pytest.raises(ValueError, match="32"):
        SegFormer.work_hw(720, 1280, 31)
    assert SegFormer.work_hw(720, 1280, 32) == (32, 32)


@pytest.mark.parametrize("script", ["image_transfer", "video_transfer"])
def test_seg_size_parser_errors(script, capsys):
    mod = __import__(script)
    parser = mod.build_parser()
    base = (["--content", "c.png"] if script == "image_transfer" else ["--video", "clip"]) + ["--style", "s.png"]
    auto = ["--auto_seg", "--synthetic_seg_weights", "--no_seg_remap"]

    def check(argv):
        args = parser.parse_args(argv)
        mod.check_seg_args(parser, args)
        return args
    with pytest.raises(SystemExit) as e:
        check(base + ["--seg_size", "512"])
    assert e.value.code == 2 and "--seg_size belongs to --auto_seg" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        check(base + auto + ["--seg_size", "16"])
    assert e.value.code == 2 and "at least 32" in capsys.readouterr().err
    assert check(base + auto + ["--seg_size", "32"]).seg_size == 32
    assert check(base + auto).seg_size is None


def test_pixel_limit_messages():
    from image_transfer import check_seg_pixels
    check_seg_pixels(None, [(4096, 4096)])
    with pytest.raises(SystemExit) as e:
        check_seg_pixels(None, [(1280, 720), (5000, 4000)])
    assert "--seg_size" in str(e.value) and "5000x4000" in str(e.value)
    check_seg_pixels(512, [(5000, 4000)])                     # the limit is on the working size
    with pytest.raises(SystemExit, match="lower --seg_size"):
        check_seg_pixels(5000, [(5000, 4000)])
    with pytest.raises(SystemExit, match="label maps"):
        check_seg_pixels(512, [(40000, 40000)])


def test_golden_file_invariants():
    from vstnet_amd.segformer import SegFormer
    from vstnet_amd.synth import synthetic_scene_u8
    g = np.load(os.path.join(REPO, "tests", "golden", "segformer_worksize.npz"))
    for case, (h, w, size, work_hw) in CASES.items():
        labels, margin = g[f"{case}.labels"], g[f"{case}.margin"].astype(np.float64)
        assert labels.shape == margin.shape == (h, w) and labels.dtype == np.uint8
        assert int(g[f"{case}.work_size"]) == size and tuple(g[f"{case}.work_hw"]) == work_hw == SegFormer.work_hw(h, w, size)
        threshold = 2 * 8 * float(g[f"{case}.e32"]) * float(g[f"{case}.max_logit"])
        close = float((margin <= threshold).mean())
        _, counts = np.unique(labels, return_counts=True)
        big = int((counts >= 0.02 * labels.size).sum())
        print(f"{case}: {100 * close:.4f} % under the threshold {threshold:.3e}, {big} labels >= 2 %")
        assert close <= 0.01 and abs(close - float(g[f"{case}.share_close"])) < 1e-3
        assert big >= 4 and big == int(g[f"{case}.labels_2pct"])
        frame = synthetic_scene_u8(h, w, int(g[f"{case}.scene_seed"]))
        assert zlib.crc32(frame.tobytes()) == int(g[f"{case}.frame_crc32"]), "synthetic_scene_u8 no longer makes the golden's frame"


def test_header_declares_the_new_entry_points():
    from vstnet_amd import _lib
    text = open(os.path.join(REPO, "include", "vstnet.h")).read()
    for name in ("vst_seg_run_scaled_u8", "vst_seg_labels_from_logits"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.EXPORTS
    m = re.search(r"#define\s+VST_SEG_MAX_LABEL_PIXELS\s+\(1LL\s*<<\s*(\d+)\)", text)
    assert m and int(m.group(1)) >= 28
    from vstnet_amd.segformer import MAX_LABEL_PIXELS, MAX_PIXELS
    L = _lib.lib()
    assert L.vst_version() >= 107 and hasattr(L, "vst_seg_run_scaled_u8") and hasattr(L, "vst_seg_labels_from_logits")
    assert MAX_LABEL_PIXELS == 1 << int(m.group(1)) and MAX_PIXELS == 1 << 24
