"""Host side of luminance preservation at the uint8 frame edge (no GPU): the two entry points exist everywhere they are
declared, their argument checks come before any launch, and video_transfer.py takes --preserve_luminance on the stubbed
stylise step, in shards and through the --gpus N launcher."""
import ctypes as C
import inspect
import os

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vst_lab_luminance_u8", "vst_lab_luminance_u8_f32")


def test_entry_points_are_declared_exported_and_built():
    from vstnet_amd import _lib
    header = open(os.path.join(REPO, "include", "vstnet.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert f"int {name}(const uint8_t* content_hwc, const float* stylized," in header
        assert name in _lib.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 7


def test_error_codes_without_a_gpu():
    from vstnet_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)         # a non-null pointer nothing dereferences: every check comes before any launch
    for name in NAMES:
        fn = getattr(L, name)
        assert fn(None, one, one, 1, 8, 8, None) == -1
        assert fn(one, None, one, 1, 8, 8, None) == -1
        assert fn(one, one, None, 1, 8, 8, None) == -1
        assert fn(one, one, one, 0, 8, 8, None) == -2
        assert fn(one, one, one, -3, 8, 8, None) == -2
        assert fn(one, one, one, 1, 0, 8, None) == -2
        assert fn(one, one, one, 65536, 8, 8, None) == -2                  # the batch is a grid dimension
        assert fn(one, one, one, 1, 8192, 8193, None) == -2                # past VST_MAX_FRAME_PIXELS
        assert fn(one, one, one, 1, 65536, 65536, None) == -2              # H * W does not fit 32 bits
    assert int(L.vst_max_frame_pixels()) == 8192 * 8192


def test_signatures():
    from vstnet_amd.color import luminance_transfer_u8
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.revresnet import RevResNet
    p = inspect.signature(FramePipeline.__init__).parameters
    assert "preserve_luminance" in p and p["preserve_luminance"].default is False
    p = inspect.signature(RevResNet.inverse_u8).parameters
    assert list(p)[1:] == ["z", "luminance_of", "scratch"] and p["luminance_of"].default is None and p["scratch"].default is None
    p = inspect.signature(luminance_transfer_u8).parameters
    assert list(p) == ["content_u8", "stylized", "out", "to_float"] and p["to_float"].default is False


def _clip(d, n):
    os.makedirs(d)
    rng = np.random.default_rng(2)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (36, 52, 3), dtype=np.uint8)).save(os.path.join(d, "%03d.png" % i))


def _read(d):
    return {f: np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))}


def test_stub_run_accepts_the_flag_and_shards_union_to_one_process(tmp_path):
    import video_transfer
    assert video_transfer.build_parser().parse_args([]).preserve_luminance is False
    _clip(tmp_path / "clip", 7)
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(tmp_path / "s.png")
    base = ["--video", str(tmp_path / "clip"), "--style", str(tmp_path / "s.png"), "--max_size", "48", "--stub_stylise",
            "--frames_only"]
    one = _read(video_transfer.main(base + ["--out_dir", str(tmp_path / "one"), "--preserve_luminance"]))
    assert sorted(one) == ["%05d.png" % i for i in range(7)]
    plain = _read(video_transfer.main(base + ["--out_dir", str(tmp_path / "plain")]))
    assert all(np.array_equal(one[f], plain[f]) for f in one)               # the stub stylises nothing: the flag is ignored
    union = {}
    for r in range(3):
        got = _read(video_transfer.main(base + ["--out_dir", str(tmp_path / ("shard%d" % r)), "--preserve_luminance",
                                                "--shard", "%d/3" % r]))
        assert not set(got) & set(union)
        union.update(got)
    assert sorted(union) == sorted(one)
    for f in one:
        assert np.array_equal(union[f], one[f]), f


def test_the_parent_of_a_multi_gpu_run_forwards_the_flag(tmp_path):
    import video_transfer
    import vstnet_amd.sharding as sh
    _clip(tmp_path / "clip", 3)
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(tmp_path / "s.png")
    seen = {}

    def fake_launch(cmds, envs):
        seen["cmds"] = cmds
        return 0
    real = sh.launch_children
    sh.launch_children = fake_launch
    try:
        argv = ["--video", str(tmp_path / "clip"), "--style", str(tmp_path / "s.png"), "--out_dir", str(tmp_path / "o"),
                "--preserve_luminance", "--gpus", "2", "--stub_stylise"]
        args = video_transfer.build_parser().parse_args(argv)
        assert args.preserve_luminance
        assert video_transfer.launch_shards(args, argv) == 0
    finally:
        sh.launch_children = real
    assert len(seen["cmds"]) == 2
    for r, cmd in enumerate(seen["cmds"]):
        child = video_transfer.build_parser().parse_args(cmd[2:])
        assert "--preserve_luminance" in cmd and child.preserve_luminance
        assert child.gpus == 1 and child.shard == "%d/2" % r
