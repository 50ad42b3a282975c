"""Per-frame style maps ("Style maps per frame"), the parts that need no GPU: the numpy restatement of
vst_style_frame against the shipped host route (Pillow's BOX + utils.style_map_weights) on float32 bit patterns, the new
export, its argument checks from the loaded library, the scripts' flags and their errors, and which planes a shard reads."""
import os

import numpy as np
import pytest
from PIL import Image

from tests import style_frames_ref as ref
from vstnet_amd import _lib

E_ARG, E_SHAPE, E_MODE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def host_route(planes, sp):
    """what load_style_map makes of planes that are at the stylised size already: PIL BOX for artistic codes, then the weights"""
    from utils.utils import style_map_weights
    imgs = [Image.fromarray(p) for p in planes]
    if sp == 1:
        imgs = [im.resize((im.size[0] // 2, im.size[1] // 2), Image.BOX) for im in imgs]
    return style_map_weights([np.asarray(im, dtype=np.uint8) for im in imgs])


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("sp", [2, 1])
@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_restatement_is_the_host_route(P, sp):
    for seed, (H, W) in enumerate([(8, 8), (12, 20), (64, 72)]):
        planes = ref.planes_of(P, H, W, 10 * P + seed, lo=1)
        got, flagged = ref.style_frame(planes, sp)
        want = host_route(planes, sp)
        assert not flagged and got.dtype == np.float32 and got.shape == want.shape == (max(P, 2),) + ((H, W) if sp == 2 else (H // 2, W // 2))
        assert np.array_equal(ref.bits(got), ref.bits(want))


@pytest.mark.parametrize("sp", [2, 1])
def test_every_pair_of_two_planes(sp):
    """K = 2: plane 0 = the row's number, plane 1 = the column's - every (v, total) pair 8-bit data can give, in one 256 x 256
    frame ((0, 0), which has no weights, stands in as (0, 1)); for artistic codes through constant 2 x 2 blocks"""
    y, x = np.mgrid[0:256, 0:256]
    planes = np.stack([y, x]).astype(np.uint8)
    planes[1, 0, 0] = 1
    if sp == 1:
        planes = np.repeat(np.repeat(planes, 2, 1), 2, 2)
    got, flagged = ref.style_frame(planes, sp)
    want = host_route(planes, sp)
    assert not flagged and got.shape == (2, 256, 256)
    assert np.array_equal(ref.bits(got), ref.bits(want))
    pairs = {(int(a), int(a) + int(b)) for a, b in zip(planes[0].reshape(-1), planes[1].reshape(-1))}
    assert len(pairs) == 256 * 256 - 1
    # the ramp form, every byte
    v = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    if sp == 1:
        v = np.repeat(np.repeat(v, 2, 1), 2, 2)
    got, flagged = ref.style_frame(v, sp)
    assert not flagged and np.array_equal(ref.bits(got), ref.bits(host_route(v, sp)))
    assert got[0].reshape(-1)[0] == 1.0 and got[1].reshape(-1)[255] == 1.0


def test_restated_zero_sum():
    planes = ref.planes_of(3, 12, 20, 5, lo=1)
    clean, flagged = ref.style_frame(planes, 2)
    assert not flagged
    planes[:, 3, 7] = 0
    got, flagged = ref.style_frame(planes, 2)
    assert flagged and got[:, 3, 7].tolist() == [1.0, 0.0, 0.0] and np.isfinite(got).all()
    got[:, 3, 7] = clean[:, 3, 7]
    assert np.array_equal(ref.bits(got), ref.bits(clean))
    with pytest.raises(ValueError, match="every plane is 0"):
        host_route(planes, 2)
    _, flagged = ref.style_frame(planes, 1)         # one pixel of a 2 x 2 block: BOX rounds up, the block's sum stays above 0
    assert not flagged
    planes[:, 2:4, 6:8] = 0
    got, flagged = ref.style_frame(planes, 1)
    assert flagged and got[:, 1, 3].tolist() == [1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_without_gpu(lib):
    assert lib.vst_version() >= 120
    header = open(os.path.join(_lib.REPO_DIR, "include", "vstnet.h")).read()
    assert "Style maps per frame (version 120" in header
    assert "vst_style_frame" in _lib.EXPORTS and hasattr(lib, "vst_style_frame") and "int vst_style_frame(" in header
    assert "#define VST_STYLE_FRAME_ZERO_SUM 1\n" in header
    # the call refuses before it touches anything (non-null addresses that nothing dereferences, far apart)
    p, d, r, f = (k << 24 for k in range(1, 5))
    call = lambda *a: lib.vst_style_frame(*a, None)      # noqa: E731
    assert call(None, 2, d, r, f, 16, 16, 2) == E_ARG
    assert call(p, 2, None, None, f, 16, 16, 2) == E_ARG
    for n in (0, -1, 9):
        assert call(p, n, d, r, f, 16, 16, 2) == E_ARG
    assert call(p + 2, 2, d, r, f, 16, 16, 2) == E_ARG and call(p, 2, d, r, f + 2, 16, 16, 2) == E_ARG
    assert call(p, 2, d + 4, r, f, 16, 16, 2) == E_ARG and call(p, 2, d, r + 8, f, 16, 16, 2) == E_ARG
    assert call(p, 2, d + 8, None, None, 16, 16, 2) == E_ARG
    for h, w in ((4, 16), (16, 4), (18, 16), (16, 18), (0, 16), (8192 * 4, 8192 * 4)):
        assert call(p, 2, d, r, f, h, w, 2) == E_SHAPE, (h, w)
    for sp in (0, 3, -1):
        assert call(p, 2, d, r, f, 16, 16, sp) == E_MODE
    # the checks come in this order
    assert call(None, 2, d, r, f, 4, 4, 0) == E_ARG and call(p, 2, d, r, f, 4, 4, 0) == E_SHAPE


def test_library_calls_refuse_without_gpu():
    import torch
    from models.cWCT import cWCT
    cpu = torch.zeros((2, 16, 24), dtype=torch.uint8)
    with pytest.raises(ValueError):
        cWCT.frame_style_map((1, 32, 16, 24), cpu)                              # not on the GPU
    with pytest.raises(ValueError):
        cWCT.frame_style_map((1, 32, 16, 24), cpu.float())
    with pytest.raises(ValueError):
        cWCT.frame_style_map((2, 32, 16, 24), cpu)                              # one frame at a time
    with pytest.raises(ValueError):
        cWCT.empty_style_map((1, 32, 16, 24), 9, "cpu")
    with pytest.raises(ValueError):
        cWCT.empty_style_map((1, 32, 16, 24), 1, "cpu")
    m = cWCT.empty_style_map((1, 128, 8, 12), 3, "cpu")                         # (buffers only: no GPU call)
    assert m.K == 3 and tuple(m.dense.shape) == tuple(m.rows.shape) == (1, 3, 96)


# ------------------------------------------------------------------------------------------------ scripts
def _rgb(path, h, w, seed):
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


@pytest.fixture()
def clip(tmp_path):
    fd = tmp_path / "clip"
    fd.mkdir()
    dirs = [tmp_path / f"w{k}" for k in range(3)]
    for i in range(5):
        _rgb(fd / f"{i:03d}.png", 16, 24, 2 + i)
    for k, d in enumerate(dirs):
        d.mkdir()
        for i in range(5):
            Image.fromarray(ref.planes_of(1, 16, 24, 20 + 5 * k + i, lo=1)[0]).save(d / f"{i:03d}.png")
    for k in range(3):
        _rgb(tmp_path / f"s{k}.png", 16, 16, k)
    Image.fromarray(ref.planes_of(1, 8, 8, 9)[0]).save(tmp_path / "m.png")
    base = ["--video", str(fd), "--out_dir", str(tmp_path / "ov"), "--stub_stylise", "--frames_only"]
    two = base + ["--styles", str(tmp_path / "s0.png"), str(tmp_path / "s1.png")]
    three = two + [str(tmp_path / "s2.png")]
    return tmp_path, two, three, [str(d) for d in dirs]


def test_parsers_accept_the_flags():
    import image_transfer
    import video_transfer
    a = video_transfer.build_parser().parse_args(["--style_map_dir", "d"])
    assert (a.style_map_dir, a.style_maps_dirs) == ("d", None)
    a = video_transfer.build_parser().parse_args(["--style_maps_dirs", "a", "b", "c"])
    assert (a.style_map_dir, a.style_maps_dirs) == (None, ["a", "b", "c"])
    a = image_transfer.build_parser().parse_args([])
    assert not hasattr(a, "style_map_dir") and not hasattr(a, "style_maps_dirs")          # one image has one map


def test_argparse_errors(clip, capsys):
    import video_transfer
    tmp, two, three, dirs = clip

    def fails(argv, *words):
        with pytest.raises(SystemExit) as e:
            video_transfer.main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err

    one = ["--style_map_dir", dirs[1]]
    auto = ["--auto_seg", "--synthetic_seg_weights", "--no_seg_remap"]
    fails(two + ["--style_map_dir", str(tmp / "nope")], "--style_map_dir", "not a directory")
    fails(three + ["--style_maps_dirs", dirs[0], str(tmp / "nope"), dirs[2]], "--style_maps_dirs", "not a directory")
    fails(two + one + ["--style_maps_dirs"] + dirs[:2], "--style_map_dir", "--style_maps_dirs", "mutually exclusive")
    fails(two + one + ["--style_map", str(tmp / "m.png")], "--style_map_dir", "--style_map", "mutually exclusive")
    fails(two + ["--style_maps_dirs"] + dirs[:2] + ["--style_maps", str(tmp / "m.png"), str(tmp / "m.png")], "--style_maps_dirs",
          "mutually exclusive")
    # K matches --styles
    fails(three + one, "--style_map_dir", "--styles A B")
    fails(two[:-3] + ["--style", str(tmp / "s0.png")] + one, "--style_map_dir", "--styles A B")
    fails(three + ["--style_maps_dirs"] + dirs[:2], "--style_maps_dirs", "2 directories for 3 styles")
    fails(two + ["--style_maps_dirs"] + dirs, "--style_maps_dirs", "3 directories for 2 styles")
    # every exclusion of --style_map
    fails(two + one + ["--alpha_s", "0.5", "0.5"], "--style_map_dir", "--alpha_s")
    fails(two + one + ["--alpha_s_end", "0.5", "0.5"], "--style_map_dir", "--alpha_s_end")
    fails(two + one + ["--content_seg", str(tmp / "m.png")], "--style_map_dir", "masked routes", "--content_seg")
    fails(two + one + ["--content_seg_dir", dirs[0]], "--style_map_dir", "masked routes")
    fails(two + one + ["--style_segs", str(tmp / "m.png"), str(tmp / "m.png")], "--style_map_dir", "masked routes")
    fails(two + one + auto, "--style_map_dir", "masked routes", "--auto_seg")
    fails(three + ["--style_maps_dirs"] + dirs + auto, "--style_maps_dirs", "masked routes", "--auto_seg")
    fails(two + one + ["--strength_labels", "1:0.5", "--content_seg", str(tmp / "m.png")], "--style_map_dir", "masked routes")
    # one map per frame in every directory, before any child starts
    os.remove(os.path.join(dirs[1], "004.png"))
    fails(two + one, "--style_map_dir", "4 maps for 5 frames")
    fails(two + one + ["--gpus", "2"], "--style_map_dir", "4 maps for 5 frames")
    fails(three + ["--style_maps_dirs"] + dirs, "--style_maps_dirs", dirs[1], "4 maps for 5 frames")
    fails(three + ["--style_maps_dirs"] + dirs + ["--gpus", "2"], "--style_maps_dirs", "4 maps for 5 frames")


def test_synthetic_motion_and_the_tiled_route_are_excluded(clip, capsys, monkeypatch):
    import video_transfer
    tmp, two, three, dirs = clip
    still = str(tmp / "clip" / "000.png")
    argv = ["--video", still, "--out_dir", str(tmp / "ov"), "--styles", str(tmp / "s0.png"), str(tmp / "s1.png"), "--temporal",
            "--synthetic_motion", "3", "--style_map_dir", dirs[0]]
    with pytest.raises(SystemExit) as e:
        video_transfer.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--synthetic_motion" in err and "--style_map_dir" in err
    # the tiled route: a frame past the whole-frame guard (the guard lowered for the test: such a frame is 64 Mpixel)
    from vstnet_amd import tiled
    monkeypatch.setattr(tiled, "max_frame_pixels", lambda: 16 * 24 - 1)
    with pytest.raises(SystemExit) as e:
        video_transfer.main(two + ["--style_map_dir", dirs[0]])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--style_map_dir" in err and "tiled route" in err


def test_a_shard_reads_its_own_planes(clip, capsys):
    """the stub rehearsal decodes what a real run decodes: the planes of a shard are those of the frames' shard_range; planes
    of another size are resized by the worker, and planes of two sizes in one frame end the run with both files' names"""
    import video_transfer
    from vstnet_amd.sharding import shard_range
    tmp, two, three, dirs = clip
    files = [sorted(os.path.join(d, f) for f in os.listdir(d)) for d in dirs]
    for world in (1, 2, 3):
        for rank in range(world):
            out = video_transfer.main(three + ["--style_maps_dirs"] + dirs + ["--shard", f"{rank}/{world}"])
            lo, hi = shard_range(5, rank, world)
            assert video_transfer.LAST_RUN["style_maps"] == {i: [f[i] for f in files] for i in range(lo, hi)}
    assert sorted(os.listdir(out)) == ["%05d.png" % i for i in range(5)]
    video_transfer.main(two + ["--style_map_dir", dirs[1]])
    assert video_transfer.LAST_RUN["style_maps"] == {i: [files[1][i]] for i in range(5)}
    for d in dirs:          # frame 2's planes at another size, all of them: resized (PIL BILINEAR) under --resize host
        Image.fromarray(ref.planes_of(1, 20, 30, 7, lo=1)[0]).save(os.path.join(d, "002.png"))
    video_transfer.main(three + ["--style_maps_dirs"] + dirs)
    Image.fromarray(ref.planes_of(1, 16, 24, 8, lo=1)[0]).save(os.path.join(dirs[2], "002.png"))
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        video_transfer.main(three + ["--style_maps_dirs"] + dirs)
    msg = str(e.value.code)
    assert "frame 2" in msg and files[0][2] in msg and files[2][2] in msg and "one size" in msg
