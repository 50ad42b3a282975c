"""CPU: the high-bit-depth edge without a GPU - the float64 reference (vstnet_amd/yuv.py) against the 8-bit reference and
against itself, DeepYuvSpec, the raw .yuv reader and writer (vstnet_amd/rawyuv.py), the C ABI's argument checks, and
`video_transfer.py --stub_stylise` on raw clips: names, sizes, bytes, shards, --out_pix_fmt behind a frame directory, the errors."""
import contextlib
import io
import os
import traceback

import numpy as np
import pytest
from PIL import Image

import yuv16_ref as R
from yuv16_ref import DeepYuvSpec, as_flat, write_raw
from vstnet_amd import _lib, yuv
from vstnet_amd.rawyuv import RawYuvClip, RawYuvWriter, merge_parts, parse_pix_fmt, pix_fmt_spec
from vstnet_amd.yuv import YuvSpec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the reference
def test_spec_shapes_enums_and_header():
    s = DeepYuvSpec("422", "bt709", "full", 10)
    assert s.codes == (_lib.YUV_422, _lib.YUV_BT709, _lib.YUV_FULL, 10) and _lib.YUV_422 == 3
    assert s.plane_shapes(3, 5) == ((3, 5), (3, 3), (3, 3)) and s.frame_bytes(3, 5) == 2 * (15 + 18)
    assert s.plane_shapes(7, 9) == ((7, 9), (7, 5), (7, 5)) and s.frame_bytes(1, 1) == 6
    assert DeepYuvSpec("420jpeg", depth=12).plane_shapes(3, 5) == ((3, 5), (2, 3), (2, 3))
    assert DeepYuvSpec("444", depth=16).frame_bytes(3, 5) == 90
    assert DeepYuvSpec("420mpeg2").frame_bytes(1080, 1920) == 1080 * 1920 * 3
    assert s == DeepYuvSpec("422", "bt709", "full", 10) and s != DeepYuvSpec("422", "bt709", "full", 12)
    assert len({s, DeepYuvSpec("422", "bt709", "full", 10)}) == 1 and "422" in repr(s) and "10" in repr(s)
    assert s != YuvSpec("444") and YuvSpec("444") != s
    for bad in (dict(layout="411"), dict(matrix="bt2020"), dict(range="wide"), dict(depth=8), dict(depth=17)):
        with pytest.raises(ValueError):
            DeepYuvSpec(**bad)
    with pytest.raises(ValueError):
        YuvSpec("422")                      # the 8-bit spec stays as it is
    flat = np.arange(s.frame_bytes(3, 5), dtype=np.uint8)
    y, u, v = s.split(flat, 3, 5)
    assert y.shape == (3, 5) and u.shape == v.shape == (3, 3) and y.dtype.itemsize == 2 and y[0, 1] == 2 + 3 * 256
    assert v[-1, -1] == int(flat[-2]) + 256 * int(flat[-1])
    with pytest.raises(ValueError):
        s.split(flat[:-2], 3, 5)
    with pytest.raises(ValueError):
        s.split(flat.astype(np.uint16), 3, 5)
    import torch
    ty, tu, tv = s.split(torch.from_numpy(flat), 3, 5)       # torch: 16-bit views too, the same bits
    assert tuple(ty.shape) == (3, 5) and tuple(tv.shape) == (3, 3) and ty.element_size() == 2
    assert np.array_equal(ty.numpy().view(np.uint16), y) and np.array_equal(tv.numpy().view(np.uint16), v)
    assert s.scales == (0.0, 1023.0, 512.0, 1023.0)
    assert DeepYuvSpec("444", "bt601", "limited", 12).scales == (256.0, 3504.0, 2048.0, 3584.0)
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    assert "#define VST_YUV_422 3\n" in hdr and "vst_yuv16_to_rgb_f32" in hdr and "vst_rgb_f32_to_yuv16" in hdr
    assert {"vst_yuv16_to_rgb_f32", "vst_rgb_f32_to_yuv16"} <= set(_lib.EXPORTS)


@pytest.mark.parametrize("depth", [10, 12, 16])
@pytest.mark.parametrize("layout", ["444", "420jpeg", "420mpeg2"])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_limited_codes_scaled_give_the_8_bit_rgb(depth, layout, matrix):
    """codes c * 2^(d-8) in limited range mean what the 8-bit codes c mean: the 8-bit reference's RGB / 255, to 1e-12"""
    H, W = 9, 13
    s8, s16 = YuvSpec(layout, matrix, "limited"), DeepYuvSpec(layout, matrix, "limited", depth)
    c = np.random.default_rng(depth).integers(0, 256, s8.frame_bytes(H, W), dtype=np.uint8)
    want = np.clip(yuv.yuv_to_rgb_float(c, H, W, s8) / 255.0, 0.0, 1.0)
    got = yuv.yuv16_to_rgb_float(as_flat(c.astype(np.uint16) << (depth - 8)), H, W, s16)
    assert got.shape == (H, W, 3) and np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("depth", [10, 16])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_full_range_444_codes_round_trip(depth, matrix):
    """codes -> RGB -> codes returns the codes, where the RGB lies inside [0, 1] (the clamp is not invertible)"""
    spec = DeepYuvSpec("444", matrix, "full", depth)
    rng = np.random.default_rng(depth)
    codes = np.empty((3, 10000), np.uint16)
    n = 0
    while n < 10000:            # random codes whose colour is inside the RGB cube
        c = rng.integers(0, spec.max_code + 1, (3, 40000), dtype=np.uint16)
        c[1:] = (spec.max_code + 1) // 2 + (c[1:].astype(np.int64) - (spec.max_code + 1) // 2) // 4
        rgb = yuv.yuv16_to_rgb_float(as_flat(c.reshape(-1)), 1, 40000, spec)
        ok = ((rgb > 0.0) & (rgb < 1.0)).all(axis=-1)[0]
        take = min(10000 - n, int(ok.sum()))
        codes[:, n:n + take] = c[:, ok][:, :take]
        n += take
    flat = as_flat(codes.reshape(-1))
    rgb = yuv.yuv16_to_rgb_float(flat, 1, 10000, spec)
    back = yuv.rgb_to_yuv16_host(rgb, spec)
    assert np.array_equal(back, flat)
    assert np.abs(yuv.rgb_to_yuv16_float(rgb, spec) - codes.reshape(-1)).max() < 1e-9


def test_422_taps_by_hand():
    spec = DeepYuvSpec("422", "bt709", "full", 10)
    u = np.array([[100, 200, 400]], np.float64)
    assert np.array_equal(yuv.upsample_chroma(u, 1, 5, "422"), [[100, 150, 200, 300, 400]])
    assert np.array_equal(yuv.upsample_chroma(u, 1, 6, "422"), [[100, 150, 200, 300, 400, 400]])
    c = np.array([[8.0, 16.0, 32.0, 64.0, 128.0]])
    assert np.array_equal(yuv.downsample_chroma(c, "422"), [[0.25 * 8 + 0.5 * 8 + 0.25 * 16, 0.25 * 16 + 0.5 * 32 + 0.25 * 64,
                                                            0.25 * 64 + 0.5 * 128 + 0.25 * 128]])
    # a constant colour survives both ways, at odd sizes
    rgb = np.full((3, 5, 3), 0.25) * [1.0, 2.0, 3.0]
    flat = yuv.rgb_to_yuv16_host(rgb, spec)
    assert flat.shape == (spec.frame_bytes(3, 5),)
    assert np.abs(yuv.yuv16_to_rgb_float(flat, 3, 5, spec) - rgb).max() < 1.5 / 1023
    f32, u8 = yuv.yuv16_to_rgb_host(flat, 3, 5, spec)
    assert f32.dtype == np.float32 and u8.dtype == np.uint8 and f32.shape == u8.shape == (3, 5, 3)
    # a code above 2^depth - 1 is limited on read
    big = as_flat(np.full(spec.frame_bytes(3, 5) // 2, 0xFFFF, np.uint16))
    top = as_flat(np.full(spec.frame_bytes(3, 5) // 2, 1023, np.uint16))
    assert np.array_equal(yuv.yuv16_to_rgb_float(big, 3, 5, spec), yuv.yuv16_to_rgb_float(top, 3, 5, spec))


def test_rule_helpers():
    assert R.near_tie(np.array([0.5, 7.5 + 2.0 ** -21, 7.5 - 2.0 ** -21])).all()
    assert not R.near_tie(np.array([0.0, 7.5 + 2.0 ** -19, 0.25])).any()
    spec = DeepYuvSpec("444", "bt709", "full", 10)
    with pytest.raises(AssertionError, match="tie"):
        R.check_codes(np.array([8], np.uint16), np.array([7.5]), spec, "tie")
    with pytest.raises(AssertionError, match="differ"):
        R.check_codes(np.array([8], np.uint16), np.array([7.4]), spec, "off by one")
    R.check_codes(np.array([7, 1023, 0], np.uint16), np.array([7.4, 2000.0, -3.0]), spec, "clamped")
    v = np.array([[[0.11, 0.73, 1.0]]])
    R.check_rgb(v.astype(np.float32).transpose(2, 0, 1), np.floor(255 * v + 0.5).astype(np.uint8), v, "ok")
    with pytest.raises(AssertionError, match="spacings"):
        R.check_rgb((v + 1e-6).astype(np.float32).transpose(2, 0, 1), None, v, "fp32 off")
    for spec in (R.SPECS_10[0], R.SPECS_DEPTHS[-1]):
        for name, flat in R.planes_cases(spec, 3, 5):
            assert flat.dtype == np.uint8 and flat.shape == (spec.frame_bytes(3, 5),), name
            R.assert_tie_free(255.0 * R.yuv16_to_rgb_float(flat, 3, 5, spec), name)
        for name, rgb in R.rgb_cases(spec, 3, 5):
            R.assert_tie_free(R.rgb_to_yuv16_float(rgb, spec), name, spec.max_code)
    # a "tie" whose two sides clamp to the same code decides nothing: full-range chroma of a saturated blue
    blue = R.rgb_to_yuv16_float(np.array([[[0.0, 0.0, 1.0]]]), DeepYuvSpec("444", "bt709", "full", 10))
    assert blue[1] == 1023.5 and not R.deciding_ties(blue, 1023).any() and R.deciding_ties(np.array([1022.5]), 1023).all()
    assert len(R.SPECS_10) == 16 and len(R.SPECS_DEPTHS) == 16


# ---------------------------------------------------------------------------------------------------------------- raw files
def test_parse_pix_fmt():
    assert parse_pix_fmt("yuv420p") == ("420", 8) and parse_pix_fmt("yuv444p") == ("444", 8)
    for fam in ("420", "422", "444"):
        for d in (9, 10, 12, 14, 16):
            assert parse_pix_fmt("yuv%sp%dle" % (fam, d)) == (fam, d)
    for bad in ("yuv422p", "yuv420p10be", "yuv420p10", "yuv420p8le", "yuv420p11le", "yuv411p", "nv12", "gray10le", "", "yuv420p10le ",
                None):
        with pytest.raises(ValueError) as e:
            parse_pix_fmt(bad)
        assert repr(bad) in str(e.value)
    assert pix_fmt_spec("yuv420p", (64, 48)) == YuvSpec("420mpeg2", "bt601", "limited")
    assert pix_fmt_spec("yuv420p", (1280, 720), siting="centre", colour_range="full") == YuvSpec("420jpeg", "bt709", "full")
    assert pix_fmt_spec("yuv422p10le", (64, 48), "bt709") == DeepYuvSpec("422", "bt709", "limited", 10)
    assert pix_fmt_spec("yuv444p16le", (64, 48), siting="centre") == DeepYuvSpec("444", "bt601", "limited", 16)


def test_clip_random_access_and_truncation(tmp_path):
    spec = DeepYuvSpec("420mpeg2", "bt601", "limited", 10)
    frames = [R.random_planes(spec, 7, 9, i) for i in range(5)]
    path = write_raw(str(tmp_path / "c.yuv"), frames)
    clip = RawYuvClip(path, 9, 7, "yuv420p10le", fps=24)
    assert len(clip) == 5 and clip.size == (9, 7) and clip.fps == 24 and clip.frame_bytes == spec.frame_bytes(7, 9)
    for i in (3, 0, 4, -1, 2):
        got = clip[i]
        assert got.dtype == np.uint8 and np.array_equal(got, frames[i]) and got is not clip[i]
    with pytest.raises(IndexError):
        clip[5]
    assert isinstance(clip.spec(), DeepYuvSpec) and clip.spec() == spec
    assert clip.spec("bt709", "full") == DeepYuvSpec("420mpeg2", "bt709", "full", 10)
    assert RawYuvClip(path, 9, 7, "yuv420p10le", siting="centre").spec().layout == "420jpeg"
    with open(path, "ab") as f:
        f.write(b"\0" * 10)
    with pytest.raises(ValueError) as e:
        RawYuvClip(path, 9, 7, "yuv420p10le")
    assert str(spec.frame_bytes(7, 9)) in str(e.value) and "10 bytes remain" in str(e.value)
    # 8-bit formats give the 8-bit spec
    p8 = write_raw(str(tmp_path / "e.yuv"), [np.zeros(YuvSpec("444").frame_bytes(7, 9), np.uint8)] * 2)
    c8 = RawYuvClip(p8, 9, 7, "yuv444p")
    assert len(c8) == 2 and type(c8.spec()) is YuvSpec and c8.spec() == YuvSpec("444", "bt601", "limited")
    assert type(RawYuvClip(p8, 18, 14, "yuv420p").spec()) is YuvSpec
    with pytest.raises(ValueError):
        RawYuvClip(p8, 9, 7, "yuv422p")


def test_writer_round_trip_and_merge(tmp_path):
    spec = DeepYuvSpec("422", "bt709", "limited", 12)
    fb = spec.frame_bytes(6, 10)
    frames = [R.random_planes(spec, 6, 10, 40 + i) for i in range(5)]
    with RawYuvWriter(str(tmp_path / "one.yuv")) as w:
        for f in frames:
            w.write(f)
        assert w.frames == 5
    clip = RawYuvClip(str(tmp_path / "one.yuv"), 10, 6, "yuv422p12le")
    assert len(clip) == 5 and all(np.array_equal(clip[i], frames[i]) for i in range(5))
    os.makedirs(tmp_path / "parts")
    parts = [str(tmp_path / "parts" / ("part_%d.yuv" % r)) for r in range(2)]
    for p, fr in zip(parts, (frames[:3], frames[3:])):          # (5 frames on 2 ranks: 3 + 2)
        write_raw(p, fr)
    with pytest.raises(RuntimeError, match="part 0"):
        merge_parts(str(tmp_path / "m.yuv"), parts[::-1], 5, fb)
    with pytest.raises(RuntimeError, match="missing"):
        merge_parts(str(tmp_path / "m.yuv"), [parts[0], str(tmp_path / "parts" / "part_9.yuv")], 5, fb)
    assert not os.path.exists(tmp_path / "m.yuv")
    merged = merge_parts(str(tmp_path / "m.yuv"), parts, 5, fb)
    assert open(merged, "rb").read() == open(tmp_path / "one.yuv", "rb").read() and not os.path.exists(tmp_path / "parts")


# -------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_refuses_bad_arguments_before_any_launch():
    """bad depth, enums, sizes and null pointers: the library's argument error, with no GPU in sight"""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    E_ARG, p = -1, 4096                     # (a non-null address: nothing dereferences it before the checks)

    def to_rgb(H=8, W=8, depth=10, layout=3, matrix=0, rng=0, ptrs=(p, p, p, p, p)):
        return L.vst_yuv16_to_rgb_f32(ptrs[0], ptrs[1], ptrs[2], H, W, depth, layout, matrix, rng, ptrs[3], ptrs[4], None)

    def to_yuv(H=8, W=8, depth=10, layout=3, matrix=0, rng=0, ptrs=(p, p, p, p)):
        return L.vst_rgb_f32_to_yuv16(ptrs[0], H, W, depth, layout, matrix, rng, ptrs[1], ptrs[2], ptrs[3], None)
    for call in (to_rgb, to_yuv):
        for kw in (dict(depth=8), dict(depth=17), dict(layout=4), dict(layout=-1), dict(matrix=2), dict(matrix=-1), dict(rng=2),
                   dict(rng=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(H=8193, W=8192)):
            assert call(**kw) == E_ARG, (call.__name__, kw)
        for k in range(4):
            a = [p] * (5 if call is to_rgb else 4)
            a[k] = None
            assert call(ptrs=tuple(a)) == E_ARG, (call.__name__, k)
    # the 8-bit calls go on refusing the new layout
    assert L.vst_yuv_to_rgb_u8(p, p, p, 8, 8, 3, 0, 0, p, None) == E_ARG
    assert L.vst_rgb_to_yuv_u8(p, 8, 8, 3, 0, 0, p, p, p, None) == E_ARG


# ---------------------------------------------------------------------------------------------------------------- the script
class _Done:
    def __init__(self, returncode, stdout, stderr):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr


def _run(args):
    """video_transfer.main(args) in this process (--stub_stylise: no GPU), reporting the exit status, stdout and stderr as a
    command line would give them"""
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


W0, H0 = 40, 56
SPEC0 = DeepYuvSpec("420mpeg2", "bt601", "limited", 10)


def smooth_frame(spec, H, W, seed):
    """a frame's bytes of a smooth picture (ramps, not noise), made with the host conversion"""
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([(xx + seed) / (W + seed), yy / H, (xx + yy) / (W + H - 1.0)], axis=-1)
    return yuv.rgb_to_yuv16_host(rgb, spec)


@pytest.fixture(scope="module")
def stub_clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("raw")
    frames = [smooth_frame(SPEC0, H0, W0, i) for i in range(3)]
    write_raw(str(d / "clip.yuv"), frames)
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(d / "s.png")
    base = ["--video", str(d / "clip.yuv"), "--style", str(d / "s.png"), "--stub_stylise", "--max_size", "64", "--pix_fmt",
            "yuv420p10le", "--video_size", "%dx%d" % (W0, H0)]
    return d, frames, base


def stub_reference(frame, in_spec, out_spec):
    """the rehearsal of a deep frame: numpy conversions on both sides, the float planes between them"""
    return yuv.rgb_to_yuv16_host(yuv.yuv16_to_rgb_host(frame, H0, W0, in_spec)[0], out_spec)


def test_script_deep_clip_in_and_out(stub_clip):
    d, frames, base = stub_clip
    p = _run(base + ["--out_dir", str(d / "one")])
    assert p.returncode == 0, p.stderr[-2000:]
    path = d / "one" / ("clip_s_%dx%d_yuv420p10le.yuv" % (W0, H0))
    assert "Save stylized video at %s" % path in p.stdout
    assert os.path.getsize(path) == 3 * SPEC0.frame_bytes(H0, W0)
    out = RawYuvClip(str(path), W0, H0, "yuv420p10le")
    for i in range(3):
        assert np.array_equal(out[i], stub_reference(frames[i], SPEC0, SPEC0)), i
    # more than 8 bits survive the trip: the luma plane keeps more than 256 levels' worth of distinct codes over the clip
    y = np.concatenate([SPEC0.split(out[i], H0, W0)[0].reshape(-1) for i in range(3)])
    assert np.abs(y.astype(np.int64) - np.concatenate([SPEC0.split(f, H0, W0)[0].reshape(-1) for f in frames])).max() <= 1
    # matrix, range and siting describe the input, and the output follows
    p = _run(base + ["--out_dir", str(d / "flags"), "--yuv_matrix", "bt709", "--yuv_range", "full", "--yuv_siting", "centre"])
    assert p.returncode == 0, p.stderr[-2000:]
    spec = DeepYuvSpec("420jpeg", "bt709", "full", 10)
    out = RawYuvClip(str(d / "flags" / path.name), W0, H0, "yuv420p10le")
    assert np.array_equal(out[1], stub_reference(frames[1], spec, spec))
    # another format on the way out
    p = _run(base + ["--out_dir", str(d / "o444"), "--out_pix_fmt", "yuv444p16le"])
    assert p.returncode == 0, p.stderr[-2000:]
    spec = DeepYuvSpec("444", "bt601", "limited", 16)
    out = RawYuvClip(str(d / "o444" / ("clip_s_%dx%d_yuv444p16le.yuv" % (W0, H0))), W0, H0, "yuv444p16le")
    assert len(out) == 3 and np.array_equal(out[2], stub_reference(frames[2], SPEC0, spec))


def test_script_shards_equal_one_process(stub_clip):
    d, frames, base = stub_clip
    p = _run(base + ["--out_dir", str(d / "whole")])
    assert p.returncode == 0, p.stderr[-2000:]
    name = "clip_s_%dx%d_yuv420p10le.yuv" % (W0, H0)
    one = open(d / "whole" / name, "rb").read()
    for r in range(2):
        p = _run(base + ["--out_dir", str(d / "sh"), "--shard", "%d/2" % r])
        assert p.returncode == 0, p.stderr[-2000:]
    parts = [str(d / "sh" / "clip_s" / ("part_%d.yuv" % r)) for r in range(2)]
    assert all(os.path.exists(q) for q in parts) and not os.path.exists(d / "sh" / name)
    merged = merge_parts(str(d / "sh" / name), parts, 3, SPEC0.frame_bytes(H0, W0))
    assert open(merged, "rb").read() == one
    p = _run(base + ["--out_dir", str(d / "g2"), "--gpus", "2"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(d / "g2" / name, "rb").read() == one and not os.path.exists(d / "g2" / "clip_s")


def test_script_png_directory_to_10_bit_422(stub_clip, tmp_path):
    from utils.utils import img_resize
    d, frames, base = stub_clip
    clip = tmp_path / "dir"
    os.makedirs(clip)
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 255, (H0, W0, 3), dtype=np.uint8) for _ in range(3)]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(clip / ("%03d.png" % i))
    args = ["--video", str(clip), "--style", str(d / "s.png"), "--stub_stylise", "--max_size", "48", "--out_dir", str(tmp_path / "o")]
    p = _run(args + ["--out_pix_fmt", "yuv422p10le", "--yuv_range", "full"])
    assert p.returncode == 0, p.stderr[-2000:]
    import video_transfer
    wsz = video_transfer.writer_size((W0, H0), 48)
    spec = DeepYuvSpec("422", "bt601", "full", 10)
    out = RawYuvClip(str(tmp_path / "o" / ("dir_s_%dx%d_yuv422p10le.yuv" % wsz)), wsz[0], wsz[1], "yuv422p10le")
    assert len(out) == 3
    for i, im in enumerate(imgs):
        want = np.asarray(img_resize(Image.fromarray(im), 48, 4).resize(wsz, Image.BICUBIC))
        assert np.array_equal(out[i], yuv.rgb_to_yuv16_host(want / 255.0, spec)), i
    # --out_format yuv alone: 8-bit 4:2:0
    p = _run(args + ["--out_format", "yuv"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = RawYuvClip(str(tmp_path / "o" / ("dir_s_%dx%d_yuv420p.yuv" % wsz)), wsz[0], wsz[1], "yuv420p")
    want = np.asarray(img_resize(Image.fromarray(imgs[0]), 48, 4).resize(wsz, Image.BICUBIC))
    assert len(out) == 3 and np.array_equal(out[0], yuv.rgb_to_yuv_host(want, YuvSpec("420mpeg2", "bt601", "limited")))
    # without the new flags nothing changes: numbered PNGs
    p = _run(args + ["--frames_only"])
    assert p.returncode == 0 and sorted(os.listdir(tmp_path / "o" / "dir_s")) == ["%05d.png" % i for i in range(3)]


def test_script_errors(stub_clip, tmp_path):
    d, frames, base = stub_clip
    head = ["--video", str(d / "clip.yuv"), "--style", str(d / "s.png"), "--stub_stylise", "--out_dir", str(tmp_path / "e")]
    p = _run(head)
    assert p.returncode == 2 and "--pix_fmt" in p.stderr and "--video_size" in p.stderr
    p = _run(head + ["--pix_fmt", "yuv420p10le"])
    assert p.returncode == 2 and "--pix_fmt" in p.stderr and "--video_size" in p.stderr
    for fmt in ("yuv422p", "yuv420p10be"):
        p = _run(head + ["--pix_fmt", fmt, "--video_size", "40x56"])
        assert p.returncode == 2 and repr(fmt) in p.stderr, p.stderr[-500:]
        p = _run(base + ["--out_dir", str(tmp_path / "e"), "--out_pix_fmt", fmt])
        assert p.returncode == 2 and repr(fmt) in p.stderr, p.stderr[-500:]
    # a deep clip that is no multiple of 4, and one above --max_size: the float resize is not built yet
    spec = DeepYuvSpec("420mpeg2", "bt601", "limited", 10)
    write_raw(str(tmp_path / "odd.yuv"), [smooth_frame(spec, 56, 42, 0)])
    p = _run(["--video", str(tmp_path / "odd.yuv"), "--style", str(d / "s.png"), "--stub_stylise", "--out_dir", str(tmp_path / "e"),
              "--pix_fmt", "yuv420p10le", "--video_size", "42x56"])
    assert p.returncode == 2 and "42x56" in p.stderr and "--max_size" in p.stderr and "multiples of 4" in p.stderr \
        and "not built yet" in p.stderr, p.stderr[-500:]
    p = _run(base + ["--out_dir", str(tmp_path / "e"), "--max_size", "48"])
    assert p.returncode == 2 and "40x56" in p.stderr and "--max_size" in p.stderr and "not built yet" in p.stderr, p.stderr[-500:]
    # a file that is not a whole number of frames
    p = _run(head + ["--pix_fmt", "yuv420p10le", "--video_size", "44x56"])
    assert p.returncode == 2 and "bytes remain" in p.stderr, p.stderr[-500:]
    # deep output is never a y4m
    p = _run(base + ["--out_dir", str(tmp_path / "e"), "--out_format", "y4m"])
    assert p.returncode == 2 and "raw .yuv" in p.stderr, p.stderr[-500:]
    assert not os.path.exists(tmp_path / "e") or not [f for f in os.listdir(tmp_path / "e") if f.endswith((".yuv", ".y4m"))]
