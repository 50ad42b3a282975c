"""The raw video edge on the GPU ("Raw video edge"): vst_yuv_to_rgb_u8 and vst_rgb_to_yuv_u8 against the
float64 restatement under the comparison rule of tests/yuv_ref.py (equal away from a tie, one count within 2^-10 of one; at
most 2 % of a case's bytes near a tie, asserted on the reference alone), with guard bytes around every output plane;
FramePipeline(src_yuv=..., out_yuv=...) bit-identical to the same pipeline around the two calls; video_transfer.py on .y4m
clips against the frame-directory route composed by hand, with shards and --gpus 2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import yuv_ref as R
from yuv_ref import YuvSpec
from vstnet_amd.synth import synthetic_state_dict
from vstnet_amd.y4m import Y4MClip, merge_parts
from vstnet_amd.yuv import rgb_to_yuv_u8, yuv_to_rgb_u8

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


# ---------------------------------------------------------------------------------------------------------------- the kernels
class Guarded:
    """uint8 device views of the given sizes carved out of one buffer pre-filled with a sentinel, `pad` bytes before, between
    and after them (pad = 64: views on the 4-byte grid; 62: on the 2-byte grid alone; 61: off both)"""

    def __init__(self, sizes, pad):
        self.sizes, self.pad = sizes, pad
        self.buf = torch.full((pad + sum(n + pad for n in sizes),), SENTINEL, dtype=torch.uint8, device="cuda")
        self.views, off = [], pad
        for n in sizes:
            self.views.append(self.buf[off:off + n])
            off += n + pad

    def check(self, what):
        host, off = self.buf.cpu().numpy(), 0
        for n in self.sizes + [0]:
            assert (host[off:off + self.pad] == SENTINEL).all(), f"{what}: bytes outside the output were written (at {off})"
            off += self.pad + n
        return [host[o:o + n] for o, n in zip(np.cumsum([self.pad] + [n + self.pad for n in self.sizes[:-1]]), self.sizes)]


def to_rgb_case(spec, H, W, flat, pad, what):
    g = Guarded([H * W * 3], pad)
    src = Guarded([int(np.prod(s)) for s in spec.plane_shapes(H, W)], pad)          # (the inputs off the grid too)
    planes = []
    for view, part in zip(src.views, spec.split(flat, H, W)):
        view.copy_(torch.from_numpy(np.ascontiguousarray(part).reshape(-1)))
        planes.append(view.view(part.shape))
    out = yuv_to_rgb_u8(tuple(planes), H, W, spec, out=g.views[0].view(H, W, 3))
    assert out.data_ptr() == g.views[0].data_ptr()
    got = g.check(what)[0].reshape(H, W, 3)
    return R.check_bytes(got, R.yuv_to_rgb_float(flat, H, W, spec), what)


def to_yuv_case(spec, H, W, rgb, pad, what):
    g = Guarded([int(np.prod(s)) for s in spec.plane_shapes(H, W)], pad)
    src = Guarded([H * W * 3], pad)
    src.views[0].copy_(torch.from_numpy(rgb.reshape(-1)))
    planes = tuple(v.view(s) for v, s in zip(g.views, spec.plane_shapes(H, W)))
    rgb_to_yuv_u8(src.views[0].view(H, W, 3), spec, out=planes)
    got = np.concatenate(g.check(what))
    return R.check_bytes(got, R.rgb_to_yuv_float(rgb, spec), what)


@pytest.mark.parametrize("spec", R.ALL_SPECS, ids=repr)
def test_kernels_against_float64(spec):
    for H, W in R.KERNEL_SHAPES:
        for pad in (64, 62, 61):
            for name, flat in R.planes_cases(spec, H, W):
                share, diff = to_rgb_case(spec, H, W, flat, pad, f"to rgb {spec} {H}x{W} {name} pad {pad}")
                print(f"to rgb {H}x{W} {name} pad {pad}: near-tie share {100 * share:.3f} %, bytes that differ {diff}")
            for name, rgb in R.rgb_cases(spec, H, W):
                share, diff = to_yuv_case(spec, H, W, rgb, pad, f"to yuv {spec} {H}x{W} {name} pad {pad}")
                print(f"to yuv {H}x{W} {name} pad {pad}: near-tie share {100 * share:.3f} %, bytes that differ {diff}")


def test_kernels_1080p_and_flat_frames():
    """one 1080 x 1920 case, through the flat Y|U|V form a y4m frame has"""
    spec, H, W = YuvSpec("420jpeg", "bt709", "limited"), 1080, 1920
    flat = R.random_planes(spec, H, W, 1)
    got = yuv_to_rgb_u8(torch.from_numpy(flat).cuda(), H, W, spec)
    assert tuple(got.shape) == (H, W, 3)
    print("to rgb 1080p: share, differ", R.check_bytes(got.cpu().numpy(), R.yuv_to_rgb_float(flat, H, W, spec), "1080p to rgb"))
    rgb = R.random_rgb(H, W, 2)
    out = rgb_to_yuv_u8(torch.from_numpy(rgb).cuda()[None], spec)
    assert tuple(out.shape) == (spec.frame_bytes(H, W),)
    print("to yuv 1080p: share, differ", R.check_bytes(out.cpu().numpy(), R.rgb_to_yuv_float(rgb, spec), "1080p to yuv"))


def test_kernels_on_side_streams():
    """one call on a non-default stream while a different call is queued on another"""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a_spec, b_spec, H, W = YuvSpec("420mpeg2", "bt601", "limited"), YuvSpec("444", "bt709", "full"), 55, 97
    flat, rgb = R.random_planes(a_spec, H, W, 31), R.random_rgb(64, 260, 32)
    d_flat, d_rgb = torch.from_numpy(flat).cuda(), torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        got_a = yuv_to_rgb_u8(d_flat, H, W, a_spec)
    with torch.cuda.stream(s2):
        got_b = rgb_to_yuv_u8(d_rgb, b_spec)
    s1.synchronize()
    s2.synchronize()
    R.check_bytes(got_a.cpu().numpy(), R.yuv_to_rgb_float(flat, H, W, a_spec), "stream 1")
    R.check_bytes(got_b.cpu().numpy(), R.rgb_to_yuv_float(rgb, b_spec), "stream 2")


def test_argument_errors_on_device_tensors():
    spec = YuvSpec()
    flat = torch.zeros(spec.frame_bytes(8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        yuv_to_rgb_u8(flat[:-1], 8, 8, spec)
    with pytest.raises(ValueError):
        yuv_to_rgb_u8(flat.cpu(), 8, 8, spec)
    with pytest.raises(ValueError):
        yuv_to_rgb_u8(flat, 8, 8, spec, out=torch.zeros((8, 9, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        rgb_to_yuv_u8(torch.zeros((8, 8, 3), dtype=torch.float32, device="cuda"), spec)
    with pytest.raises(ValueError):
        rgb_to_yuv_u8(torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"), spec, out=flat[:-2])


# --------------------------------------------------------------------------------------------------------------- the pipeline
H_, W_, N_ = 64, 96, 7
IN_SPEC, OUT_SPEC = YuvSpec("420mpeg2", "bt601", "limited"), YuvSpec("420jpeg", "bt709", "full")


@pytest.fixture(scope="module")
def net():
    from models.RevResNet import RevResNet
    n = RevResNet(hidden_dim=16, sp_steps=2)
    n.load_state_dict(synthetic_state_dict(1234, 16, 2))
    return n.to("cuda").eval()


@pytest.fixture(scope="module")
def cw():
    from models.cWCT import cWCT
    return cWCT()


@pytest.fixture(scope="module")
def s_stats(net, cw):
    from vstnet_amd.synth import synthetic_scene_u8
    with torch.no_grad():
        return cw.style_stats(net.forward_u8(torch.from_numpy(synthetic_scene_u8(48, 64, 77)).cuda()[None]))


def smooth_planes(spec, H, W, seed):
    """a frame's planes of a smooth synthetic scene (a stylisable picture, not noise), made with the host conversion"""
    from vstnet_amd.synth import synthetic_scene_u8
    return R.rgb_to_yuv_host(synthetic_scene_u8(H, W, seed), spec)


def rgb_of(flats, H, W, spec):
    return [yuv_to_rgb_u8(torch.from_numpy(f).cuda(), H, W, spec).cpu().numpy() for f in flats]


def run(pipe, frames, **kw):
    got = {}
    assert pipe.run(frames, lambda i, a: got.__setitem__(i, a.copy()), **kw) == len(frames)
    return [got[i] for i in sorted(got)]


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (what, i)


@pytest.mark.parametrize("resize", [False, True], ids=["same size", "device resize"])
@pytest.mark.parametrize("lum", [False, True], ids=["plain", "luminance"])
def test_pipeline_src_yuv_equals_rgb_frames(net, cw, s_stats, resize, lum):
    """planes in = the RGB frames yuv_to_rgb_u8 gives for them in; 7 frames through 3 slots on 2 streams, so slots are reused
    (with preserve_luminance the RGB slot is read after the decode: the `consumed` ordering)"""
    from vstnet_amd.pipeline import FramePipeline
    Hs, Ws = (130, 194) if resize else (H_, W_)
    flats = [smooth_planes(IN_SPEC, Hs, Ws, 200 + i) for i in range(N_)]
    frames = rgb_of(flats, Hs, Ws, IN_SPEC)
    kw = dict(depth=3, compute_streams=2, preserve_luminance=lum)
    if resize:
        kw.update(src_height=Hs, src_width=Ws, max_size=96)
    tf = lambda z, i: cw.transfer_with_stats(z, s_stats)                           # noqa: E731
    want = run(FramePipeline(net, tf, H_, W_, **kw), frames)
    pipe = FramePipeline(net, tf, H_, W_, src_yuv=IN_SPEC, **kw)
    assert tuple(pipe.h_in.shape) == (3, IN_SPEC.frame_bytes(Hs, Ws)) and tuple(pipe.d_yuv.shape) == tuple(pipe.h_in.shape)
    same(run(pipe, flats), want, "src_yuv")
    same(run(pipe, flats[::-1]), want[::-1], "src_yuv, a second run")
    assert len({w.tobytes() for w in want}) == N_ and want[0].shape == (H_, W_, 3)
    with pytest.raises(ValueError):
        pipe.run([frames[0]], lambda i, a: None)            # an RGB frame is not what this pipeline takes


def test_pipeline_out_yuv_equals_conversion_of_rgb_frames(net, cw, s_stats):
    from vstnet_amd.pipeline import FramePipeline
    flats = [smooth_planes(IN_SPEC, H_, W_, 220 + i) for i in range(N_)]
    frames = rgb_of(flats, H_, W_, IN_SPEC)
    tf = lambda z, i: cw.transfer_with_stats(z, s_stats)                           # noqa: E731
    kw = dict(depth=3, compute_streams=2)
    plain = run(FramePipeline(net, tf, H_, W_, **kw), frames)
    want = [rgb_to_yuv_u8(torch.from_numpy(f).cuda(), OUT_SPEC).cpu().numpy() for f in plain]
    same(run(FramePipeline(net, tf, H_, W_, out_yuv=OUT_SPEC, **kw), frames), want, "out_yuv")
    same(run(FramePipeline(net, tf, H_, W_, src_yuv=IN_SPEC, out_yuv=OUT_SPEC, **kw), flats), want, "src_yuv and out_yuv")
    assert want[0].shape == (OUT_SPEC.frame_bytes(H_, W_),)
    # without the keywords: no new buffer
    p = FramePipeline(net, tf, H_, W_, **kw)
    assert p.d_yuv is None and p.d_out_yuv is None and tuple(p.h_in.shape) == (3, H_, W_, 3) == tuple(p.h_out.shape)


def test_pipeline_stats_window_with_warmup_both_ways(net, cw, s_stats):
    from vstnet_amd.pipeline import FramePipeline
    flats = [smooth_planes(IN_SPEC, H_, W_, 240 + i) for i in range(N_)]
    frames = rgb_of(flats, H_, W_, IN_SPEC)
    tf = lambda z, i, **k: cw.transfer_with_stats(z, s_stats, **k)                 # noqa: E731
    kw = dict(depth=3, compute_streams=2, stats_window=3, stats_decay=0.5, frame_stats=lambda z, out=None: cw.frame_stats(z, None, out=out))
    whole = run(FramePipeline(net, tf, H_, W_, **kw), frames)
    warm = run(FramePipeline(net, tf, H_, W_, **kw), frames[2:], start_index=2, warmup=frames[:2])
    same(warm, whole[2:], "the window's warm-up frames (RGB)")
    want = [rgb_to_yuv_u8(torch.from_numpy(f).cuda(), OUT_SPEC).cpu().numpy() for f in whole]
    pipe = FramePipeline(net, tf, H_, W_, src_yuv=IN_SPEC, out_yuv=OUT_SPEC, **kw)
    same(run(pipe, flats[2:], start_index=2, warmup=flats[:2]), want[2:], "the window with warm-up frames, planes both ways")
    same(run(pipe, flats), want, "the window, planes both ways")
    cold = run(FramePipeline(net, tf, H_, W_, **kw), frames[2:], start_index=2)
    assert not np.array_equal(cold[0], whole[2])            # the warm-up frames matter


# ------------------------------------------------------------------------------------------------------------------ the script
CW, CH, CN = 96, 64, 6


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    from vstnet_amd.synth import synthetic_scene_u8
    d = tmp_path_factory.mktemp("y4m_gpu")
    spec = YuvSpec("420mpeg2", "bt601", "limited")
    flats = [smooth_planes(spec, CH, CW, 300 + i) for i in range(CN)]
    R.write_y4m(str(d / "clip.y4m"), flats, CW, CH, "C420mpeg2")
    Image.fromarray(synthetic_scene_u8(72, 104, 50)).save(d / "s.png")
    return d, spec, flats


def script_args(d, *more):
    return ["--video", str(d / "clip.y4m"), "--style", str(d / "s.png"), "--synthetic_weights", "--max_size", "64"] + list(more)


def frames_of(path):
    c = Y4MClip(path)
    return c, [c[i] for i in range(len(c))]


def test_script_y4m_equals_the_frame_directory_route(clip, tmp_path):
    import video_transfer
    d, spec, flats = clip
    out = video_transfer.main(script_args(d, "--out_dir", str(tmp_path / "o")))
    assert out == str(tmp_path / "o" / "clip_s.y4m")
    got, got_frames = frames_of(out)
    wsz = video_transfer.writer_size((CW, CH), 64)
    assert len(got) == CN and got.size == wsz and got.layout == "420mpeg2" and got.colour_range == "limited" and got.fps == 25
    # by hand: PNGs of the device-converted frames, the frame-directory route with the device resize, its PNGs converted
    fd = tmp_path / "frames"
    fd.mkdir()
    for i, f in enumerate(rgb_of(flats, CH, CW, spec)):
        Image.fromarray(f).save(fd / ("%03d.png" % i))
    pngs = video_transfer.main(["--video", str(fd), "--style", str(d / "s.png"), "--synthetic_weights", "--max_size", "64",
                                "--resize", "device", "--frames_only", "--out_dir", str(tmp_path / "p")])
    for i in range(CN):
        rgb = np.asarray(Image.open(os.path.join(pngs, "%05d.png" % i)).convert("RGB"))
        assert rgb.shape == (wsz[1], wsz[0], 3)
        want = rgb_to_yuv_u8(torch.from_numpy(np.array(rgb)).cuda(), spec).cpu().numpy()
        assert np.array_equal(got_frames[i], want), i
    assert len({f.tobytes() for f in got_frames}) == CN


@pytest.mark.parametrize("flags", [[], ["--stats_window", "3", "--preserve_luminance"]], ids=["plain", "window and luminance"])
def test_script_shards_and_gpus_equal_one_process(clip, tmp_path, flags):
    import video_transfer
    d, spec, flats = clip
    one = open(video_transfer.main(script_args(d, "--out_dir", str(tmp_path / "one"), *flags)), "rb").read()
    for r in range(2):
        part = video_transfer.main(script_args(d, "--out_dir", str(tmp_path / "sh"), "--shard", "%d/2" % r, *flags))
        assert part == str(tmp_path / "sh" / "clip_s" / ("part_%d.yuv" % r))
    wsz = video_transfer.writer_size((CW, CH), 64)
    merged = merge_parts(str(tmp_path / "sh" / "clip_s.y4m"), [str(tmp_path / "sh" / "clip_s" / ("part_%d.yuv" % r)) for r in range(2)],
                         CN, wsz[0], wsz[1], 25, spec)
    assert open(merged, "rb").read() == one
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py")] + script_args(d, "--out_dir", str(tmp_path / "g2"),
                                                                                             "--gpus", "2", *flags),
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(tmp_path / "g2" / "clip_s.y4m", "rb").read() == one
    if flags:
        plain = open(video_transfer.main(script_args(d, "--out_dir", str(tmp_path / "plain"))), "rb").read()
        assert plain != one and len(plain) == len(one)          # the flags reach the frames


def test_script_auto_seg_on_a_y4m_input(clip, tmp_path):
    import video_transfer
    d, spec, flats = clip
    out = video_transfer.main(script_args(d, "--out_dir", str(tmp_path / "o"), "--auto_seg", "--synthetic_seg_weights", "--seg_variant",
                                          "b1", "--no_seg_remap", "--save_seg_label"))
    c = Y4MClip(out)
    from vstnet_amd.resize import img_resize_size
    sty = img_resize_size((CW, CH), 64, 4)
    assert len(c) == CN
    for i in range(CN):
        m = np.asarray(Image.open(tmp_path / "o" / "segmentation" / ("%05d_label.png" % i)))
        assert m.shape == (sty[1], sty[0]) and m.dtype == np.uint8
