"""Per-frame strength maps, the parts that need no GPU: the numpy restatement of Pillow's BOX and 8-bit
BILINEAR against Pillow itself, the library's bilinear table against the restated one, the new exports and their argument
checks, strength_table's parsing, the scripts' flags and their errors, and which mattes a shard reads."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from PIL import Image

from tests import strength_frames_ref as ref
from vstnet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["vst_strength_frame", "vst_resize_coeffs_u8_bilinear", "vst_resize_grey_u8"]
E_ARG, E_SHAPE, E_MODE = -1, -2, -3
# (source h, w) -> (destination h, w): a shrink, an enlargement, one axis unchanged, the largest shrink allowed
RESIZES = [((23, 37), (12, 16)), ((12, 16), (28, 40)), ((23, 37), (23, 16)), ((256, 256), (16, 16))]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the restatement is Pillow's
@pytest.mark.parametrize("src,dst", RESIZES)
def test_restated_bilinear_is_pillows(src, dst):
    for seed in (0, 1):
        img = ref.grey(src[0], src[1], seed)
        want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
        assert np.array_equal(ref.pil_resize_grey(img, (dst[1], dst[0])), want)


@pytest.mark.parametrize("h,w", [(8, 8), (12, 20), (64, 48)])
def test_restated_box_is_pillows(h, w):
    for seed in (0, 1):
        img = ref.grey(h, w, seed)
        want = np.asarray(Image.fromarray(img).resize((w // 2, h // 2), Image.BOX))
        assert np.array_equal(ref.box2(img), want)
    # (the one-pass mean is another function: the two-pass form is what the kernel must compute)
    a = img.astype(np.int32)
    one_pass = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    assert not np.array_equal(one_pass, want)


def test_restated_frame_is_the_host_route(tmp_path):
    """a matte through the restatement = load_strength_map of the same image (what bind_strength is given), both modes"""
    from image_transfer import load_strength_map
    img = ref.grey(24, 40, 3)
    Image.fromarray(img).save(tmp_path / "m.png")
    for mode, sp in (("photorealistic", 2), ("artistic", 1)):
        assert np.array_equal(ref.strength_frame(img, None, None, sp), load_strength_map(str(tmp_path / "m.png"), (40, 24), mode))
    big = ref.pil_resize_grey(img, (80, 48))
    assert np.array_equal(ref.strength_frame(big, None, None, 1), load_strength_map(str(tmp_path / "m.png"), (80, 48), "artistic"))


def test_rows_of_restates_the_cell_order():
    H, W = 8, 12
    idx = np.arange(H * W, dtype=np.float32).reshape(H, W)
    r = ref.rows_of(idx, H, W, 2)
    assert sorted(r.tolist()) == list(range(H * W))
    assert r[:8].tolist() == [0, 1, 12, 13, 2, 3, 14, 15]                   # half 0, cell (0, 0): rows 0-1 of the cell
    assert r[H * W // 2] == 2 * W                                           # half 1 starts at row 2 of the cell
    r1 = ref.rows_of(np.arange(24, dtype=np.float32).reshape(4, 6), H, W, 1)
    assert r1[:6].tolist() == [0, 1, 2, 3, 4, 5] and r1[6] == 12 and r1[12] == 6    # half 0: code row 0 of every cell; half 1: row 1


# ------------------------------------------------------------------------------------------------ the library, host side
@pytest.mark.parametrize("src,dst", RESIZES)
def test_bilinear_table_is_the_restated_one(lib, src, dst):
    from vstnet_amd import resize
    for a, b in zip(src, dst):
        ks, bounds, kk = resize.coeffs_u8_bilinear(a, b)
        rks, rbounds, rkk = ref.pil_coeffs_bilinear(a, b)
        assert ks == rks and np.array_equal(bounds, rbounds) and np.array_equal(kk, rkk), (a, b)
    ks = C.c_int(0)
    assert lib.vst_resize_coeffs_u8_bilinear(257, 16, C.byref(ks), None, None) == E_SHAPE
    assert lib.vst_resize_coeffs_u8_bilinear(0, 16, C.byref(ks), None, None) == E_ARG
    assert lib.vst_resize_coeffs_u8_bilinear(256, 16, C.byref(ks), None, None) == 0 and ks.value == 33


def test_new_exports(lib):
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    assert lib.vst_version() >= 110
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.vst_strength_frame.argtypes) == 9 and len(lib.vst_resize_grey_u8.argtypes) == 9


def test_new_calls_check_their_arguments_before_any_launch(lib):
    fake, odd = C.c_void_p(4096), C.c_void_p(4098)
    sf = lib.vst_strength_frame
    assert sf(None, None, fake, fake, fake, 16, 16, 2, None) == E_ARG             # no input
    assert sf(fake, None, None, None, None, 16, 16, 2, None) == E_ARG             # no output
    assert sf(None, fake, None, fake, None, 16, 16, 2, None) == E_ARG             # labels without a table
    assert sf(odd, None, None, fake, None, 16, 16, 2, None) == E_ARG              # a byte map off the dword grid
    assert sf(fake, None, None, C.c_void_p(4100), None, 16, 16, 2, None) == E_ARG
    assert sf(fake, None, None, fake, None, 16, 18, 2, None) == E_SHAPE
    assert sf(fake, None, None, fake, None, 4, 16, 2, None) == E_SHAPE
    assert sf(fake, fake, fake, fake, fake, 16, 16, 3, None) == E_MODE
    assert sf(fake, fake, fake, fake, fake, 16, 16, 0, None) == E_MODE
    rg = lib.vst_resize_grey_u8
    assert rg(None, 16, 16, fake, 8, 8, fake, fake, None) == E_ARG
    assert rg(fake, 16, 16, fake, 8, 8, None, fake, None) == E_ARG                # a pass runs: tables needed
    assert rg(fake, 16, 16, fake, 8, 8, fake, None, None) == E_ARG                # two passes: tmp needed
    assert rg(fake, 0, 16, fake, 8, 8, fake, fake, None) == E_ARG
    assert rg(fake, 16, 257, fake, 8, 16, fake, fake, None) == E_SHAPE            # a shrink past 16x


def test_strength_table_parsing():
    import torch
    from models.cWCT import cWCT
    t = cWCT.strength_table("12:0.2, 20:0")
    assert t.dtype == torch.float32 and tuple(t.shape) == (256,) and not t.is_cuda
    want = np.ones(256, np.float32)
    want[12], want[20] = np.float32(0.2), 0.0
    assert np.array_equal(t.numpy(), want)
    assert np.array_equal(cWCT.strength_table({12: 0.2, 20: 0}).numpy(), want)
    d = cWCT.strength_table({3: 1.0}, default=0.25).numpy()
    assert d[3] == 1.0 and d[0] == np.float32(0.25) and d[255] == np.float32(0.25)
    assert np.array_equal(cWCT.strength_table("").numpy(), np.ones(256, np.float32))
    for bad in ("256:0.5", "-1:0.5", "3:1.5", "3:-0.1", "3:nan", "3", "a:0.5", "3:0.5:1", {2.5: 0.5}):
        with pytest.raises(ValueError):
            cWCT.strength_table(bad)
    with pytest.raises(ValueError):
        cWCT.strength_table("3:0.5", default=1.5)


def test_frame_strength_rejects_bad_arguments():
    import torch
    from models.cWCT import cWCT
    cpu = torch.zeros((16, 24), dtype=torch.uint8)
    with pytest.raises(ValueError):
        cWCT.frame_strength((1, 32, 16, 24))                                       # neither input
    with pytest.raises(ValueError):
        cWCT.frame_strength((1, 32, 16, 24), matte=cpu)                            # not on the GPU
    with pytest.raises(ValueError):
        cWCT.frame_strength((2, 32, 16, 24), matte=cpu)                            # one frame at a time
    with pytest.raises(ValueError):
        cWCT.frame_strength((1, 24, 16, 24), matte=cpu)                            # no packed form
    with pytest.raises(ValueError):
        cWCT.frame_strength((1, 32, 16, 24), matte=cpu.float())


# ------------------------------------------------------------------------------------------------ scripts
def _rgb(path, h, w, seed):
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


@pytest.fixture()
def clip(tmp_path):
    fd, md = tmp_path / "clip", tmp_path / "mattes"
    fd.mkdir()
    md.mkdir()
    for i in range(5):
        _rgb(fd / f"{i:03d}.png", 16, 24, 2 + i)
        Image.fromarray(ref.grey(16, 24, 20 + i)).save(md / f"{i:03d}.png")
    _rgb(tmp_path / "s.png", 16, 16, 1)
    Image.fromarray(ref.grey(8, 8, 9)).save(tmp_path / "m.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--out_dir", str(tmp_path / "ov"), "--stub_stylise",
            "--frames_only"]
    return tmp_path, base, md


def test_parsers_accept_the_flags():
    import image_transfer
    import video_transfer
    a = video_transfer.build_parser().parse_args(["--strength_dir", "d", "--strength_labels", "1:0.5", "--strength_default", "0.5"])
    assert (a.strength_dir, a.strength_labels, a.strength_default) == ("d", "1:0.5", 0.5)
    a = video_transfer.build_parser().parse_args([])
    assert (a.strength_dir, a.strength_labels, a.strength_default) == (None, None, 1.0)
    a = image_transfer.build_parser().parse_args(["--strength_labels", "1:0.5"])
    assert a.strength_labels == "1:0.5" and not hasattr(a, "strength_dir")


def test_argparse_errors(clip, capsys):
    import image_transfer
    import video_transfer
    tmp, base, md = clip

    def fails(main, argv, *words):
        with pytest.raises(SystemExit) as e:
            main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err

    fails(video_transfer.main, base + ["--strength_dir", str(tmp / "nope")], "--strength_dir", "not a directory")
    os.remove(md / "004.png")
    fails(video_transfer.main, base + ["--strength_dir", str(md)], "--strength_dir", "4 maps for 5 frames")
    fails(video_transfer.main, base + ["--strength_dir", str(md), "--gpus", "2"], "--strength_dir")    # before any child starts
    Image.fromarray(ref.grey(16, 24, 0)).save(md / "004.png")
    fails(video_transfer.main, base + ["--strength_dir", str(md), "--strength_map", str(tmp / "m.png")], "mutually exclusive")
    fails(video_transfer.main, base + ["--strength_labels", "12:0.2"], "--strength_labels", "--content_seg")
    fails(video_transfer.main, base + ["--strength_default", "0.5"], "--strength_default")
    img = ["--content", str(tmp / "s.png"), "--style", str(tmp / "s.png"), "--synthetic_weights", "--out_dir", str(tmp / "o")]
    fails(image_transfer.main, img + ["--strength_labels", "12:0.2"], "--strength_labels", "--content_seg")
    fails(image_transfer.main, img + ["--strength_labels", "300:0.2", "--content_seg", str(tmp / "m.png")], "--strength_labels", "0..255")
    fails(image_transfer.main, img + ["--strength_labels", "3:0.2", "--content_seg", str(tmp / "m.png"), "--mode", "artistic"],
          "photorealistic")


def test_a_shard_reads_its_own_mattes(clip):
    """the stub rehearsal decodes what a real run decodes: the mattes of a shard are those of the frames' shard_range"""
    import video_transfer
    from vstnet_amd.sharding import shard_range
    tmp, base, md = clip
    files = sorted(str(md / f) for f in os.listdir(md))
    for world in (1, 2, 3):
        for rank in range(world):
            out = video_transfer.main(base + ["--strength_dir", str(md), "--shard", f"{rank}/{world}"])
            lo, hi = shard_range(5, rank, world)
            assert video_transfer.LAST_RUN["mattes"] == {i: files[i] for i in range(lo, hi)}
    assert sorted(os.listdir(out)) == ["%05d.png" % i for i in range(5)]
    # mattes of another size are resized (PIL BILINEAR) by the worker under --resize host
    Image.fromarray(ref.grey(20, 30, 7)).save(md / "002.png")
    video_transfer.main(base + ["--strength_dir", str(md)])
