"""CPU: the raw video edge without a GPU - the float64 reference of the Y'CbCr conversions (vstnet_amd/yuv.py) checked
against hand values and Pillow, the YUV4MPEG2 reader and writer (vstnet_amd/y4m.py), and `video_transfer.py --stub_stylise`
on .y4m clips: header, frame count, shards, --gpus 2, a frame-directory input with --out_format y4m, the errors."""
import os
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

import yuv_ref
from yuv_ref import ALL_SPECS, YuvSpec, write_y4m
from vstnet_amd import _lib, yuv
from vstnet_amd.y4m import Y4MClip, Y4MError, Y4MWriter, header_line, merge_parts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the reference
def test_spec_shapes_and_enums():
    s = YuvSpec("420mpeg2", "bt709", "full")
    assert s.codes == (_lib.YUV_420_LEFT, _lib.YUV_BT709, _lib.YUV_FULL)
    assert YuvSpec().codes == (_lib.YUV_420_CENTRE, _lib.YUV_BT601, _lib.YUV_LIMITED)
    assert s.plane_shapes(3, 5) == ((3, 5), (2, 3), (2, 3)) and s.frame_bytes(3, 5) == 27
    assert YuvSpec("444").plane_shapes(3, 5) == ((3, 5),) * 3 and YuvSpec("444").frame_bytes(1, 1) == 3
    assert s.frame_bytes(1080, 1920) == 1080 * 1920 * 3 // 2 and s.frame_bytes(1, 1) == 3
    with pytest.raises(ValueError):
        YuvSpec("422")
    with pytest.raises(ValueError):
        s.split(np.zeros(26, np.uint8), 3, 5)
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    for name, val in (("VST_YUV_444", 0), ("VST_YUV_420_CENTRE", 1), ("VST_YUV_420_LEFT", 2), ("VST_YUV_BT601", 0),
                      ("VST_YUV_BT709", 1), ("VST_YUV_LIMITED", 0), ("VST_YUV_FULL", 1)):
        assert "#define %s %d\n" % (name, val) in hdr


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """bad enums, bad sizes and null pointers: the library's argument error, with no GPU in sight"""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    E_ARG, p = -1, 4096                     # (a non-null address: nothing dereferences it before the checks)
    assert L.vst_yuv_to_rgb_u8(p, p, p, 8, 8, 3, 0, 0, p, None) == E_ARG            # layout
    assert L.vst_yuv_to_rgb_u8(p, p, p, 8, 8, -1, 0, 0, p, None) == E_ARG
    assert L.vst_yuv_to_rgb_u8(p, p, p, 8, 8, 0, 2, 0, p, None) == E_ARG            # matrix
    assert L.vst_yuv_to_rgb_u8(p, p, p, 8, 8, 0, 0, 2, p, None) == E_ARG            # range
    assert L.vst_yuv_to_rgb_u8(p, p, p, 0, 8, 0, 0, 0, p, None) == E_ARG            # sizes
    assert L.vst_yuv_to_rgb_u8(p, p, p, 8, -3, 0, 0, 0, p, None) == E_ARG
    assert L.vst_yuv_to_rgb_u8(p, p, p, 8193, 8192, 0, 0, 0, p, None) == E_ARG      # past VST_MAX_FRAME_PIXELS
    for k in range(4):                                                              # null pointers
        a = [p, p, p, p]
        a[k] = None
        assert L.vst_yuv_to_rgb_u8(a[0], a[1], a[2], 8, 8, 1, 0, 0, a[3], None) == E_ARG
        assert L.vst_rgb_to_yuv_u8(a[0], 8, 8, 1, 0, 0, a[1], a[2], a[3], None) == E_ARG
    assert L.vst_rgb_to_yuv_u8(p, 8, 8, 3, 0, 0, p, p, p, None) == E_ARG
    assert L.vst_rgb_to_yuv_u8(p, 8, 8, 2, 5, 0, p, p, p, None) == E_ARG
    assert L.vst_rgb_to_yuv_u8(p, 8, 8, 2, 1, 7, p, p, p, None) == E_ARG
    assert L.vst_rgb_to_yuv_u8(p, 8, 0, 2, 1, 1, p, p, p, None) == E_ARG
    assert b"argument" in L.vst_error_string(E_ARG).lower() or L.vst_error_string(E_ARG)


@pytest.mark.parametrize("spec", ALL_SPECS, ids=repr)
def test_neutral_greys_are_exact_both_ways(spec):
    """R = G = B <-> U = V = 128, in every matrix / range pair and layout: the grey axis maps onto itself exactly"""
    H, W = 5, 7
    lo, hi = (16, 235) if spec.range == "limited" else (0, 255)
    for code in (lo, hi, (lo + hi) // 2, lo + 1):
        flat = np.full(spec.frame_bytes(H, W), 128, np.uint8)
        flat[:H * W] = code
        rgb = yuv.yuv_to_rgb_host(flat, H, W, spec)
        assert (rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 1] == rgb[..., 2]).all()
        want = np.clip(np.floor((code - lo) * 255.0 / (hi - lo) + 0.5), 0, 255)
        assert (rgb == want).all()
        back = yuv.rgb_to_yuv_host(rgb, spec)
        assert (back[H * W:] == 128).all() and (back[:H * W] == code).all()


def test_full_range_bt601_444_against_pillow():
    """Pillow's YCbCr is full-range BT.601 in fixed point: within one count, each way (measured: 1 and 1)"""
    rgb = yuv_ref.random_rgb(36, 52, 3)
    spec = YuvSpec("444", "bt601", "full")
    ours = yuv.rgb_to_yuv_host(rgb, spec).reshape(3, 36, 52).transpose(1, 2, 0)
    pil = np.asarray(Image.fromarray(rgb).convert("YCbCr"))
    d = int(np.abs(ours.astype(int) - pil.astype(int)).max())
    print("rgb -> ycbcr against Pillow: max difference", d)
    assert d <= 1
    back = yuv.yuv_to_rgb_host(np.ascontiguousarray(pil.transpose(2, 0, 1)).reshape(-1), 36, 52, spec)
    pil_back = np.asarray(Image.merge("YCbCr", [Image.fromarray(np.ascontiguousarray(pil[..., k])) for k in range(3)]).convert("RGB"))
    d = int(np.abs(back.astype(int) - pil_back.astype(int)).max())
    print("ycbcr -> rgb against Pillow: max difference", d)
    assert d <= 1


@pytest.mark.parametrize("matrix", ("bt601", "bt709"))
@pytest.mark.parametrize("rng,bound", (("full", 1), ("limited", 2)))
def test_444_round_trip(matrix, rng, bound):
    """RGB -> 4:4:4 -> RGB: one rounding each way; limited range has 219 luma codes for 256 values (measured: 1 and 2)"""
    rgb = yuv_ref.random_rgb(36, 52, 5)
    spec = YuvSpec("444", matrix, rng)
    back = yuv.yuv_to_rgb_host(yuv.rgb_to_yuv_host(rgb, spec), 36, 52, spec)
    d = int(np.abs(back.astype(int) - rgb.astype(int)).max())
    print(matrix, rng, "round trip: max difference", d)
    assert d <= bound


def test_chroma_taps_by_hand_3x5():
    """a 3 x 5 luma frame has 2 x 3 chroma planes: the bilinear taps, the clamps at the borders and the odd sizes, by hand"""
    p = np.array([[0.0, 40.0, 80.0], [100.0, 140.0, 180.0]])
    # centre siting: luma column x sits at chroma (x - 1/2) / 2 = -1/4, 1/4, 3/4, 5/4, 7/4; row y at -1/4, 1/4, 3/4
    cols = np.array([[0, 10, 30, 50, 70.0], [100, 110, 130, 150, 170.0]])        # per chroma row; x = 0 clamps to sample 0
    want = np.stack([cols[0], 0.75 * cols[0] + 0.25 * cols[1], 0.25 * cols[0] + 0.75 * cols[1]])
    assert np.array_equal(yuv.upsample_chroma(p, 3, 5, "420jpeg"), want)
    # left siting: column x sits at chroma x / 2 = 0, 1/2, 1, 3/2, 2
    cols = np.array([[0, 20, 40, 60, 80.0], [100, 120, 140, 160, 180.0]])
    want = np.stack([cols[0], 0.75 * cols[0] + 0.25 * cols[1], 0.25 * cols[0] + 0.75 * cols[1]])
    assert np.array_equal(yuv.upsample_chroma(p, 3, 5, "420mpeg2"), want)
    # down: rows (0, 1) and (2, 2 again); columns (0, 1), (2, 3), (4, 4 again) - or [1/4 1/2 1/4] around 0, 2, 4, edges replicated
    c = np.array([[0, 8, 16, 24, 32.0], [40, 48, 56, 64, 72.0], [80, 88, 96, 104, 112.0]])
    assert np.array_equal(yuv.downsample_chroma(c, "420jpeg"), np.array([[24.0, 40, 52], [84, 100, 112]]))
    left_rows = np.stack([0.25 * c[:, [0, 1, 3]] + 0.5 * c[:, [0, 2, 4]] + 0.25 * c[:, [1, 3, 4]]])[0]
    assert np.array_equal(left_rows[0], [2.0, 16, 30])
    assert np.array_equal(yuv.downsample_chroma(c, "420mpeg2"), np.stack([0.5 * (left_rows[0] + left_rows[1]), left_rows[2]]))
    # single-sample planes: 1 x 1 and 2 x 2 frames read the one sample everywhere
    for layout in ("420jpeg", "420mpeg2"):
        assert np.array_equal(yuv.upsample_chroma(np.array([[7.0]]), 2, 2, layout), np.full((2, 2), 7.0))
        assert np.array_equal(yuv.downsample_chroma(np.array([[1.0, 3.0], [5.0, 7.0]]), layout),
                              [[4.0]] if layout == "420jpeg" else [[0.5 * (1.5 + 5.5)]])


def test_tie_helper_and_rule():
    v = np.array([0.5, 1.5 - 2.0 ** -11, 1.5 + 2.0 ** -9, 2.25, 300.5, -7.5])
    assert yuv.near_tie(v).tolist() == [True, True, False, False, True, True]
    assert yuv.round_bytes(v).tolist() == [1, 1, 2, 2, 255, 0]
    ok = np.full(200, 2.25)
    ok[0] = 0.5
    assert yuv_ref.check_bytes(np.r_[0, [2] * 199].astype(np.uint8), ok) == (0.005, 1)       # a near-tie byte may go either way
    with pytest.raises(AssertionError):
        yuv_ref.check_bytes(np.r_[1, 3, [2] * 198].astype(np.uint8), ok)                     # any other byte may not
    with pytest.raises(AssertionError):
        yuv_ref.check_bytes(np.array([1], np.uint8), np.array([0.5]))                        # a case of ties alone is no case


# ------------------------------------------------------------------------------------------------------- reader and writer
W0, H0 = 52, 36
SPEC0 = YuvSpec("420mpeg2", "bt601", "limited")


def _frames(n, spec=SPEC0, W=W0, H=H0):
    fr = [yuv_ref.random_planes(spec, H, W, 100 + i) for i in range(n)]
    for i, f in enumerate(fr):
        f[:4] = i
    return fr


@pytest.mark.parametrize("tag,extra,params,layout,rng", [
    ("C420jpeg", "", "", "420jpeg", None), ("C420mpeg2", " XCOLORRANGE=FULL", "", "420mpeg2", "full"),
    ("C420", " XYSCSS=420 XCOLORRANGE=LIMITED", " Ip", "420jpeg", "limited"), ("C444", "", " Xfoo=1 Ybar", "444", None),
    ("", "", "", "420jpeg", None)])
def test_reader_accepts(tmp_path, tag, extra, params, layout, rng):
    spec = YuvSpec(layout)
    frames = _frames(3, spec)
    clip = Y4MClip(write_y4m(str(tmp_path / "a.y4m"), frames, W0, H0, tag, extra, params))
    assert len(clip) == 3 and clip.size == (W0, H0) and clip.layout == layout and clip.colour_range == rng
    assert clip.fps == Fraction(25, 1) and clip.frame_bytes == spec.frame_bytes(H0, W0)
    for i in (2, 0, 1, -1):                                 # random access
        got = clip[i]
        assert got.dtype == np.uint8 and got.shape == (clip.frame_bytes,) and np.array_equal(got, frames[i])
    with pytest.raises(IndexError):
        clip[3]
    assert clip.spec().range == (rng or "limited") and clip.spec().matrix == "bt601"
    assert clip.spec("bt709", "full") == YuvSpec(layout, "bt709", "full")


def test_reader_header_variants(tmp_path):
    path = str(tmp_path / "b.y4m")
    fr = _frames(2, YuvSpec("420jpeg"), 1280, 2)
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 H2 W1280 F30000:1001 I? A0:0\n")         # any order, no C, unknown interlacing, NTSC rate
        for a in fr:
            f.write(b"FRAME\n" + a.tobytes())
    clip = Y4MClip(path)
    assert clip.fps == Fraction(30000, 1001) and clip.size == (1280, 2) and len(clip) == 2 and np.array_equal(clip[1], fr[1])
    assert clip.spec().matrix == "bt709"                              # auto: 1280 wide


@pytest.mark.parametrize("tag,extra,word", [
    ("C420paldv", "", "C420paldv"), ("Cmono", "", "Cmono"), ("Cmono16", "", "Cmono16"), ("C422", "", "C422"), ("C411", "", "C411"),
    ("C420p10", "", "C420p10"), ("C444p12", "", "C444p12"), ("C420p16", "", "C420p16"), ("C420jpeg", " It", "It"),
    ("C420jpeg", " Ib", "Ib"), ("C420jpeg", " Im", "Im"), ("C420jpeg", " XCOLORRANGE=WIDE", "XCOLORRANGE=WIDE")])
def test_reader_rejects_naming_the_token(tmp_path, tag, extra, word):
    path = write_y4m(str(tmp_path / "c.y4m"), _frames(1), W0, H0, tag, extra)
    with pytest.raises(Y4MError, match=word):
        Y4MClip(path)


def test_reader_truncation_and_missing_marker(tmp_path):
    frames = _frames(3)
    good = open(write_y4m(str(tmp_path / "d.y4m"), frames, W0, H0), "rb").read()
    per = 6 + SPEC0.frame_bytes(H0, W0)
    for name, data, msg in (("cut.y4m", good[:-10], "frame 2 is truncated"),                     # inside the last frame's planes
                            ("cut2.y4m", good[:len(good) - per + 6], "frame 2 is truncated"),    # right after its FRAME line
                            ("marker.y4m", good[:len(good) - per] + b"FRUME\n" + good[len(good) - per + 6:], "frame 2: no FRAME marker"),
                            ("short.y4m", good[:len(good) - per + 3], "frame 2: no FRAME marker"),
                            ("magic.y4m", b"YUV4MPEG " + good[10:], "not a YUV4MPEG2"),
                            ("nosize.y4m", b"YUV4MPEG2 W52 F25:1\n", "W and H")):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(Y4MError, match=msg):
            Y4MClip(str(p))


def test_writer_round_trip_and_merge(tmp_path):
    frames = _frames(5)
    one = str(tmp_path / "one.y4m")
    with Y4MWriter(one, W0, H0, 25, SPEC0) as w:
        for f in frames:
            w.write(f)
        with pytest.raises(ValueError):
            w.write(frames[0][:-1])
    data = open(one, "rb").read()
    assert data.startswith(b"YUV4MPEG2 W52 H36 F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\nFRAME\n")
    assert header_line(8, 8, Fraction(30000, 1001), YuvSpec("444", "bt709", "full")) == \
        b"YUV4MPEG2 W8 H8 F30000:1001 Ip A1:1 C444 XCOLORRANGE=FULL\n"
    clip = Y4MClip(one)
    assert len(clip) == 5 and clip.layout == "420mpeg2" and clip.colour_range == "limited"
    assert all(np.array_equal(clip[i], frames[i]) for i in range(5))
    # headerless parts of 3 + 2 frames behind one header: the same bytes, the parts removed
    os.makedirs(tmp_path / "parts")
    parts = [str(tmp_path / "parts" / ("part_%d.yuv" % r)) for r in range(2)]
    for p, chunk in zip(parts, (frames[:3], frames[3:])):
        with Y4MWriter(p, W0, H0, 25, SPEC0, header=False) as w:
            for f in chunk:
                w.write(f)
    merged = merge_parts(str(tmp_path / "m.y4m"), parts, 5, W0, H0, 25, SPEC0)
    assert open(merged, "rb").read() == data and not os.path.exists(tmp_path / "parts")
    # a part of the wrong length: an error, nothing written
    os.makedirs(tmp_path / "parts")
    for p, chunk in zip(parts, (frames[:2], frames[3:])):
        with Y4MWriter(p, W0, H0, 25, SPEC0, header=False) as w:
            for f in chunk:
                w.write(f)
    with pytest.raises(RuntimeError, match="part 0"):
        merge_parts(str(tmp_path / "m2.y4m"), parts, 5, W0, H0, 25, SPEC0)
    assert not os.path.exists(tmp_path / "m2.y4m")


# ------------------------------------------------------------------------------------------------------------- the script
class _Done:
    def __init__(self, returncode, stdout, stderr):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr


def _run(args):
    """video_transfer.main(args) in this process (the children of --gpus N are processes of their own): exit status, stdout and
    stderr as a command line would give them"""
    import contextlib
    import io
    import traceback
    import video_transfer
    out, err, rc = io.StringIO(), io.StringIO(), 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            video_transfer.main(list(args))
        except SystemExit as e:
            rc = e.code if isinstance(e.code, int) else 1
        except Exception:       # noqa: BLE001 - what the interpreter would print before it exits with status 1
            traceback.print_exc()
            rc = 1
    return _Done(rc, out.getvalue(), err.getvalue())


@pytest.fixture(scope="module")
def stub_clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("y4m")
    frames = _frames(6)
    write_y4m(str(d / "clip.y4m"), frames, W0, H0, "C420mpeg2", " XCOLORRANGE=FULL")
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(d / "s.png")
    base = ["--video", str(d / "clip.y4m"), "--style", str(d / "s.png"), "--stub_stylise", "--max_size", "48"]
    p = _run(base + ["--out_dir", str(d / "one")])
    assert p.returncode == 0, p.stderr[-2000:]
    return d, frames, base, p


def test_script_y4m_in_y4m_out(stub_clip):
    from utils.utils import img_resize
    from video_transfer import writer_size
    d, frames, base, p = stub_clip
    assert "--resize device is in force" in p.stderr         # the default, --resize host, does not hold for a y4m input
    out = Y4MClip(str(d / "one" / "clip_s.y4m"))
    wsz = writer_size((W0, H0), 48)
    # the input's layout and range (the header's FULL), its rate since --fps was not given, the writer size
    assert len(out) == 6 and out.size == wsz and out.layout == "420mpeg2" and out.colour_range == "full" and out.fps == 25
    spec = YuvSpec("420mpeg2", "bt601", "full")
    for i in range(6):          # the rehearsal: numpy conversions around the host resizes
        rgb = Image.fromarray(yuv.yuv_to_rgb_host(frames[i], H0, W0, spec))
        want = yuv.rgb_to_yuv_host(np.asarray(img_resize(rgb, 48, 4).resize(wsz, Image.BICUBIC)), spec)
        assert np.array_equal(out[i], want), i
    assert "Save stylized video at %s" % (d / "one" / "clip_s.y4m") in p.stdout


def test_script_shards_and_gpus_equal_one_process(stub_clip):
    d, frames, base, _ = stub_clip
    one = open(d / "one" / "clip_s.y4m", "rb").read()
    for r in range(2):
        p = _run(base + ["--out_dir", str(d / "sh"), "--shard", "%d/2" % r])
        assert p.returncode == 0, p.stderr[-2000:]
    parts = [str(d / "sh" / "clip_s" / ("part_%d.yuv" % r)) for r in range(2)]
    assert all(os.path.exists(q) for q in parts) and not os.path.exists(d / "sh" / "clip_s.y4m")
    wsz = Y4MClip(str(d / "one" / "clip_s.y4m")).size
    merged = merge_parts(str(d / "sh" / "clip_s.y4m"), parts, 6, wsz[0], wsz[1], 25, YuvSpec("420mpeg2", "bt601", "full"))
    assert open(merged, "rb").read() == one
    p = _run(base + ["--out_dir", str(d / "g2"), "--gpus", "2"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(d / "g2" / "clip_s.y4m", "rb").read() == one and not os.path.exists(d / "g2" / "clip_s")


def test_script_flags_and_frame_directory(stub_clip, tmp_path):
    d, frames, base, _ = stub_clip
    # the flags describe the input, and the output follows: limited overrides the header, --fps the rate
    p = _run(base + ["--out_dir", str(tmp_path / "o"), "--yuv_range", "limited", "--yuv_matrix", "bt709", "--fps", "24",
                     "--resize", "device"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--resize device is in force" not in p.stderr
    out = Y4MClip(str(tmp_path / "o" / "clip_s.y4m"))
    assert out.colour_range == "limited" and out.fps == 24
    spec = YuvSpec("420mpeg2", "bt709", "limited")
    from utils.utils import img_resize
    rgb = Image.fromarray(yuv.yuv_to_rgb_host(frames[0], H0, W0, spec))
    assert np.array_equal(out[0], yuv.rgb_to_yuv_host(np.asarray(img_resize(rgb, 48, 4).resize(out.size, Image.BICUBIC)), spec))
    # a frame directory with --out_format y4m: C420jpeg, limited, --fps (default 30); without the flag nothing changes
    clip = tmp_path / "dir"
    os.makedirs(clip)
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 255, (H0, W0, 3), dtype=np.uint8) for _ in range(3)]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(clip / ("%03d.png" % i))
    args = ["--video", str(clip), "--style", str(d / "s.png"), "--stub_stylise", "--max_size", "48", "--out_dir", str(tmp_path / "o2")]
    p = _run(args + ["--out_format", "y4m", "--yuv_range", "full"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = Y4MClip(str(tmp_path / "o2" / "dir_s.y4m"))
    assert len(out) == 3 and out.layout == "420jpeg" and out.colour_range == "full" and out.fps == 30
    spec = YuvSpec("420jpeg", "bt601", "full")
    for i, im in enumerate(imgs):
        want = np.asarray(img_resize(Image.fromarray(im), 48, 4).resize(out.size, Image.BICUBIC))
        assert np.array_equal(out[i], yuv.rgb_to_yuv_host(want, spec)), i
    p = _run(args + ["--frames_only"])
    assert p.returncode == 0 and sorted(os.listdir(tmp_path / "o2" / "dir_s")) == ["%05d.png" % i for i in range(3)]


def test_script_errors(stub_clip, tmp_path):
    d, frames, base, _ = stub_clip
    for flags, word in ((["--yuv_matrix", "bt2020"], "--yuv_matrix"), (["--yuv_range", "wide"], "--yuv_range"),
                        (["--out_format", "mkv"], "--out_format")):
        p = _run(base + ["--out_dir", str(tmp_path / "e")] + flags)
        assert p.returncode == 2 and word in p.stderr, p.stderr[-500:]
    # a frame outside the device resize's limits: an error that says so, no host fallback
    big = yuv_ref.random_planes(SPEC0, 4, 400, 1)
    write_y4m(str(tmp_path / "wide.y4m"), [big], 400, 4)
    p = _run(["--video", str(tmp_path / "wide.y4m"), "--style", str(d / "s.png"), "--stub_stylise", "--max_size", "16",
              "--out_dir", str(tmp_path / "e")])
    assert p.returncode == 2 and "outside the device resize's limits" in p.stderr, p.stderr[-500:]
    # an unsupported clip: the reader's error names the token
    write_y4m(str(tmp_path / "i.y4m"), _frames(1), W0, H0, "C422")
    p = _run(["--video", str(tmp_path / "i.y4m"), "--style", str(d / "s.png"), "--stub_stylise", "--out_dir", str(tmp_path / "e")])
    assert p.returncode != 0 and "C422" in p.stderr
    # without cv2 the message for any other file names the way out
    try:
        import cv2  # noqa: F401
    except ImportError:
        import video_transfer
        with pytest.raises(RuntimeError, match=r"\.y4m"):
            video_transfer.read_frames(str(tmp_path / "clip.avi"))
