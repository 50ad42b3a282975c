"""The high-bit-depth edge on the GPU ("High-bit-depth edge"): vst_yuv16_to_rgb_f32 and vst_rgb_f32_to_yuv16
against the float64 restatement under the rule of tests/yuv16_ref.py (codes and bytes EQUAL floor(v64 + 0.5), every case free of
near-ties by construction; fp32 planes within one spacing), on aligned and offset bases, flat and as planes, with every byte
around the outputs guarded; FramePipeline with a DeepYuvSpec on either side bit-identical to the same library calls made one
frame at a time; what the feature is for - more than 256 luma levels survive the loop; video_transfer.py on raw clips."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import yuv16_ref as R
from yuv16_ref import DeepYuvSpec
from vstnet_amd.rawyuv import RawYuvClip, merge_parts
from vstnet_amd.synth import synthetic_state_dict
from vstnet_amd.yuv import YuvSpec, rgb_f32_to_yuv16, rgb_to_yuv16_host, yuv16_to_rgb_f32

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


# ---------------------------------------------------------------------------------------------------------------- the kernels
class Carved:
    """uint8 device views of the given byte sizes carved out of one buffer pre-filled with a sentinel.  Every view starts
    `shift` bytes past a multiple of 256 and at least 256 bytes lie before, between and after the views; check() asserts that
    every byte outside the views still holds the sentinel and returns the views' bytes."""

    def __init__(self, sizes, shift):
        self.spans, off = [], 256
        for n in sizes:
            self.spans.append((off + shift, n))
            off = (off + shift + n + 255) // 256 * 256 + 256
        self.buf = torch.full((off,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.views = [self.buf[o:o + n] for o, n in self.spans]

    def check(self, what):
        host = self.buf.cpu().numpy()
        outside = np.ones(host.shape, bool)
        for o, n in self.spans:
            outside[o:o + n] = False
        assert (host[outside] == SENTINEL).all(), f"{what}: bytes outside the output were written"
        return [host[o:o + n].copy() for o, n in self.spans]


def plane_tensors(spec, H, W, flat_np, shift, as_planes):
    """the frame on the device, on bases `shift` bytes off the 256-byte grid: one flat uint8 tensor, or three 16-bit planes"""
    if not as_planes:
        c = Carved([flat_np.size], shift)
        c.views[0].copy_(torch.from_numpy(flat_np))
        return c, c.views[0]
    parts = spec.split(flat_np, H, W)
    c = Carved([2 * p.size for p in parts], shift)
    planes = []
    for view, part in zip(c.views, parts):
        view.copy_(torch.from_numpy(np.ascontiguousarray(part).view(np.uint8).reshape(-1)))
        planes.append(view.view(torch.int16).view(part.shape))
    return c, tuple(planes)


def to_rgb_case(spec, H, W, flat, v64, off_grid, as_planes, what):
    """(the u16 planes 2 bytes, the fp32 planes 4 bytes, the u8 frame 2 bytes) off their grids when off_grid"""
    _, src = plane_tensors(spec, H, W, flat, 2 if off_grid else 0, as_planes)
    f = Carved([12 * H * W], 4 if off_grid else 0)
    b = Carved([3 * H * W], 2 if off_grid else 0)
    out = yuv16_to_rgb_f32(src, H, W, spec, out=f.views[0].view(torch.float32).view(1, 3, H, W), out_u8=b.views[0].view(H, W, 3))
    assert out.data_ptr() == f.views[0].data_ptr() and tuple(out.shape) == (1, 3, H, W)
    got_f = f.check(what)[0].view(np.float32).reshape(3, H, W)
    got_b = b.check(what)[0].reshape(H, W, 3)
    return R.check_rgb(got_f, got_b, v64, what)


def to_yuv_case(spec, H, W, rgb, v64, off_grid, as_planes, what):
    src = Carved([12 * H * W], 4 if off_grid else 0)
    x = src.views[0].view(torch.float32).view(1, 3, H, W)
    x.copy_(torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1)))[None])
    shapes = spec.plane_shapes(H, W)
    if as_planes:
        g = Carved([2 * s[0] * s[1] for s in shapes], 2 if off_grid else 0)
        rgb_f32_to_yuv16(x, spec, out=tuple(v.view(torch.int16).view(s) for v, s in zip(g.views, shapes)))
    else:
        g = Carved([spec.frame_bytes(H, W)], 2 if off_grid else 0)
        assert rgb_f32_to_yuv16(x, spec, out=g.views[0]).data_ptr() == g.views[0].data_ptr()
    R.check_codes(np.concatenate(g.check(what)).view("<u2"), v64, spec, what)


@pytest.mark.parametrize("spec", R.SPECS_10 + R.SPECS_DEPTHS, ids=repr)
def test_kernels_against_float64(spec):
    worst = 0.0
    for H, W in R.shapes_of(spec):
        for name, flat in R.planes_cases(spec, H, W):
            v64 = R.yuv16_to_rgb_float(flat, H, W, spec)        # (the reference once per case, shared by the four runs)
            for off_grid in (False, True):
                for as_planes in (False, True):
                    worst = max(worst, to_rgb_case(spec, H, W, flat, v64, off_grid, as_planes,
                                                   f"to rgb {spec} {H}x{W} {name} off_grid={off_grid} planes={as_planes}"))
        for name, rgb in R.rgb_cases(spec, H, W):
            v64 = R.rgb_to_yuv16_float(rgb, spec)
            for off_grid in (False, True):
                for as_planes in (False, True):
                    to_yuv_case(spec, H, W, rgb, v64, off_grid, as_planes,
                                f"to yuv {spec} {H}x{W} {name} off_grid={off_grid} planes={as_planes}")
    print(f"{spec}: largest fp32 error {worst:.3f} spacings")


def test_u8_output_is_optional_and_changes_nothing():
    """rgb_hwc_u8 NULL is not an error (the one argument check that needs a launch), and the float planes are the same bits"""
    spec, H, W = DeepYuvSpec("420jpeg", "bt601", "limited", 12), 55, 97
    flat = R.planes_cases(spec, H, W)[0][1]
    d = torch.from_numpy(flat).cuda()
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    with_u8 = yuv16_to_rgb_f32(d, H, W, spec, out_u8=u8)
    without = yuv16_to_rgb_f32(d, H, W, spec)
    assert torch.equal(with_u8, without)
    R.check_rgb(without[0].cpu().numpy(), u8.cpu().numpy(), R.yuv16_to_rgb_float(flat, H, W, spec), "optional u8")


def test_kernels_on_side_streams():
    """one call on a non-default stream while a different call is queued on another"""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a_spec, b_spec = DeepYuvSpec("420mpeg2", "bt601", "limited", 10), DeepYuvSpec("422", "bt709", "full", 16)
    flat = R.planes_cases(a_spec, 55, 97)[0][1]
    rgb = R.rgb_cases(b_spec, 64, 260)[0][1]
    d_flat, d_rgb = torch.from_numpy(flat).cuda(), torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1))).cuda()[None]
    u8 = torch.empty((55, 97, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        got_a = yuv16_to_rgb_f32(d_flat, 55, 97, a_spec, out_u8=u8)
    with torch.cuda.stream(s2):
        got_b = rgb_f32_to_yuv16(d_rgb, b_spec)
    s1.synchronize()
    s2.synchronize()
    R.check_rgb(got_a[0].cpu().numpy(), u8.cpu().numpy(), R.yuv16_to_rgb_float(flat, 55, 97, a_spec), "stream 1")
    R.check_codes(got_b.cpu().numpy().view("<u2"), R.rgb_to_yuv16_float(rgb, b_spec), b_spec, "stream 2")


def test_argument_errors_on_device_tensors():
    spec = DeepYuvSpec()
    flat = torch.zeros(spec.frame_bytes(8, 8), dtype=torch.uint8, device="cuda")
    x = torch.zeros((1, 3, 8, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        yuv16_to_rgb_f32(flat[:-2], 8, 8, spec)
    with pytest.raises(ValueError):
        yuv16_to_rgb_f32(flat.cpu(), 8, 8, spec)
    with pytest.raises(ValueError):
        yuv16_to_rgb_f32(flat, 8, 8, spec, out=torch.zeros((1, 3, 8, 9), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        yuv16_to_rgb_f32(flat, 8, 8, spec, out_u8=torch.zeros((8, 9, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        yuv16_to_rgb_f32(flat, 8, 8, YuvSpec())             # the 8-bit spec belongs to the 8-bit calls
    with pytest.raises(ValueError):
        rgb_f32_to_yuv16(x.to(torch.uint8), spec)
    with pytest.raises(ValueError):
        rgb_f32_to_yuv16(x, spec, out=flat[:-2])
    with pytest.raises(ValueError):
        rgb_f32_to_yuv16(x.cpu(), spec)


# --------------------------------------------------------------------------------------------------------------- the pipeline
H_, W_, N_ = 56, 40, 4
DEEP_IN, DEEP_OUT = DeepYuvSpec("420mpeg2", "bt601", "limited", 10), DeepYuvSpec("422", "bt709", "full", 12)


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


def scene(H, W, seed):
    from vstnet_amd.synth import synthetic_scene_u8
    return synthetic_scene_u8(H, W, seed)


def deep_frame(spec, H, W, seed):
    """a frame's bytes of a smooth synthetic scene (a stylisable picture, not noise), made with the host conversion; the scene
    is given a fractional part so that the codes are not multiples of 2^(depth - 8)"""
    rgb = (scene(H, W, seed).astype(np.float64) + np.random.default_rng(seed).uniform(0, 1, (H, W, 3))) / 256.0
    return rgb_to_yuv16_host(rgb, spec)


def run(pipe, frames, **kw):
    got = {}
    assert pipe.run(frames, lambda i, a: got.__setitem__(i, a.copy()), **kw) == len(frames)
    return [got[i] for i in sorted(got)]


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (what, i)


def serial(net, cw, s_stats, frames, src=None, out=None, lum=False, window=1, decay=0.5, out_hw=None):
    """One stream, one frame at a time, the library calls the pipeline is documented to make.  frames: flat deep frames under
    `src`, else uint8 RGB frames."""
    from vstnet_amd.color import luminance_transfer, luminance_transfer_u8
    from vstnet_amd.resize import resize_f32
    ring, outs = [], []
    with torch.no_grad():
        for f in frames:
            if src is not None:
                u8 = torch.empty((1, H_, W_, 3), dtype=torch.uint8, device="cuda")
                x = yuv16_to_rgb_f32(torch.from_numpy(f).cuda(), H_, W_, src, out_u8=u8)
                z = net(x)
            else:
                u8 = torch.from_numpy(f).cuda()[None]
                z = net.forward_u8(u8)
            kw = {}
            if window > 1:
                ring = ([cw.frame_stats(z, None)] + ring)[:window]
                pooled = cw.pool_stats(ring, decay=decay)
                kw = dict(content_stats=lambda rec, b: pooled)
            z_cs = cw.transfer_with_stats(z, s_stats, **kw)
            if out is None:
                outs.append(net.inverse_u8(z_cs, luminance_of=u8 if lum else None)[0].cpu().numpy())
                continue
            sty = net._inverse(z_cs)
            if lum:
                sty = luminance_transfer(x, sty) if src is not None else luminance_transfer_u8(u8, sty, to_float=True)
            if out_hw is not None:
                sty = resize_f32(sty, out_hw)
            outs.append(rgb_f32_to_yuv16(sty, out).cpu().numpy())
    return outs


def pipeline(net, cw, s_stats, window=1, **kw):
    from vstnet_amd.pipeline import FramePipeline
    if window > 1:
        kw.update(stats_window=window, stats_decay=0.5, frame_stats=lambda z, out=None: cw.frame_stats(z, None, out=out))
    return FramePipeline(net, lambda z, i, **k: cw.transfer_with_stats(z, s_stats, **k), H_, W_, depth=3, compute_streams=2, **kw)


@pytest.mark.parametrize("mode", ["plain", "luminance", "window"])
@pytest.mark.parametrize("sides", ["deep in", "deep out", "deep in and out"])
def test_pipeline_equals_the_calls_one_frame_at_a_time(net, cw, s_stats, sides, mode):
    """4 frames through 3 slots on 2 streams, so a slot is reused; then a second run of the same pipeline, frames reversed"""
    src = DEEP_IN if "in" in sides else None
    out = DEEP_OUT if "out" in sides else None
    frames = [deep_frame(DEEP_IN, H_, W_, 400 + i) if src is not None else scene(H_, W_, 400 + i) for i in range(N_)]
    lum, window = mode == "luminance", 3 if mode == "window" else 1
    want = serial(net, cw, s_stats, frames, src, out, lum, window)
    spec_kw = {k: v for k, v in (("src_yuv", src), ("out_yuv", out)) if v is not None}
    pipe = pipeline(net, cw, s_stats, window, preserve_luminance=lum, **spec_kw)
    if src is not None:
        assert tuple(pipe.h_in.shape) == (3, DEEP_IN.frame_bytes(H_, W_)) and tuple(pipe.d_xf.shape) == (3, 1, 3, H_, W_)
    if out is not None:
        assert tuple(pipe.h_out.shape) == (3, DEEP_OUT.frame_bytes(H_, W_)) and want[0].shape == (DEEP_OUT.frame_bytes(H_, W_),)
    same(run(pipe, frames), want, f"{sides}, {mode}")
    same(run(pipe, frames[::-1]), serial(net, cw, s_stats, frames[::-1], src, out, lum, window), f"{sides}, {mode}, a second run")
    assert len({w.tobytes() for w in want}) == N_


def test_pipeline_deep_out_at_another_size(net, cw, s_stats):
    frames = [scene(H_, W_, 420 + i) for i in range(N_)]
    Ho, Wo = 84, 52
    want = serial(net, cw, s_stats, frames, None, DEEP_OUT, True, out_hw=(Ho, Wo))
    pipe = pipeline(net, cw, s_stats, out_yuv=DEEP_OUT, out_height=Ho, out_width=Wo, preserve_luminance=True)
    same(run(pipe, frames), want, "deep out, resized")
    assert want[0].shape == (DEEP_OUT.frame_bytes(Ho, Wo),)


def test_pipeline_constructor_errors_and_untouched_defaults(net, cw, s_stats):
    from vstnet_amd.pipeline import FramePipeline
    tf = lambda z, i: cw.transfer_with_stats(z, s_stats)                           # noqa: E731
    with pytest.raises(ValueError, match="follow-up"):
        FramePipeline(net, tf, H_, W_, src_yuv=DEEP_IN, src_height=2 * H_, src_width=2 * W_, max_size=56)
    with pytest.raises(ValueError, match="decode hook"):
        FramePipeline(net, tf, H_, W_, out_yuv=DEEP_OUT, decode=lambda z: net.inverse_u8(z))
    with pytest.raises(ValueError):
        FramePipeline(net, tf, H_, W_, src_yuv="yuv420p10le")
    p = FramePipeline(net, tf, H_, W_, depth=3)        # without the keywords: no new buffer
    assert p.d_yuv is None and p.d_out_yuv is None and p.d_xf is None and p.d_of is None and p.d_of_rs is None
    assert tuple(p.h_in.shape) == (3, H_, W_, 3) == tuple(p.h_out.shape)
    with pytest.raises(ValueError):
        pipeline(net, cw, s_stats, src_yuv=DEEP_IN).run([scene(H_, W_, 1)], lambda i, a: None)     # an RGB frame is not its input


def test_more_than_256_levels_survive_the_loop(net):
    """What the edge is for.  Identity transform, 4:4:4 full-range 10-bit frames of a smooth ramp with more than 600 distinct Y
    codes, deep in and deep out: the output keeps more than 256 distinct Y codes - impossible through the 8-bit edge by
    construction - and differs from the input by at most 2 codes: the project's frame budget of 1e-3 of full scale is 1.02
    ten-bit codes, plus the rounding."""
    from vstnet_amd.pipeline import FramePipeline
    spec = DeepYuvSpec("444", "bt709", "full", 10)
    yy, xx = np.mgrid[0:H_, 0:W_].astype(np.float64)
    frames = []
    for i in range(N_):
        ramp = 0.1 + 0.8 * (yy * W_ + xx + 3 * i) / (H_ * W_ + 3 * N_)            # 2240 pixels; Y spans 0.8 x 0.914 x 1023 = 748 codes
        frames.append(rgb_to_yuv16_host(np.stack([ramp, ramp * 0.9 + 0.05, ramp * 0.8 + 0.1], axis=-1), spec))
    y_in = [spec.split(f, H_, W_)[0] for f in frames]
    assert all(len(np.unique(y)) > 600 for y in y_in)
    got = run(FramePipeline(net, lambda z, i: z, H_, W_, depth=3, compute_streams=2, src_yuv=spec, out_yuv=spec), frames)
    diff = np.concatenate([np.abs(g.view("<u2").astype(np.int64) - f.view("<u2").astype(np.int64)) for g, f in zip(got, frames)])
    levels = [len(np.unique(spec.split(g, H_, W_)[0])) for g in got]
    print(f"deep loop, identity transform: {100.0 * float((diff != 0).mean()):.3f} % of the samples differ, by at most "
          f"{int(diff.max())} codes; distinct Y codes per frame {levels}")
    assert min(levels) > 256
    assert diff.max() <= 2


# ------------------------------------------------------------------------------------------------------------------ the script
CW, CH, CN = 40, 56, 6


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("raw_gpu")
    flats = [deep_frame(DEEP_IN, CH, CW, 500 + i) for i in range(CN)]
    R.write_raw(str(d / "clip.yuv"), flats)
    Image.fromarray(scene(72, 104, 50)).save(d / "s.png")
    return d, flats


def script_args(d, *more):
    return ["--video", str(d / "clip.yuv"), "--pix_fmt", "yuv420p10le", "--video_size", "%dx%d" % (CW, CH), "--style",
            str(d / "s.png"), "--synthetic_weights", "--max_size", "64"] + list(more)


def script_style(d):
    """the network, the cWCT and the style statistics as video_transfer.py makes them"""
    from image_transfer import build_network
    from models.cWCT import cWCT
    from utils.utils import img_resize, to_tensor_u8
    net = build_network("photorealistic", None, True, torch.device("cuda"), None)
    cw = cWCT()
    with torch.no_grad():
        z_s = net.forward_u8(to_tensor_u8(img_resize(Image.open(d / "s.png").convert("RGB"), 64, down_scale=4)).cuda())
        return net, cw, cw.style_stats(z_s)


NAME = "clip_s_%dx%d_yuv420p10le.yuv" % (CW, CH)


@pytest.fixture(scope="module")
def one_process(clip, tmp_path_factory):
    import video_transfer
    d, flats = clip
    o = tmp_path_factory.mktemp("one")
    out = video_transfer.main(script_args(d, "--out_dir", str(o)))
    assert out == str(o / NAME)
    return open(out, "rb").read()


def test_script_raw_clip_equals_the_pipeline(clip, one_process):
    from vstnet_amd.pipeline import FramePipeline
    d, flats = clip
    net, cw, s_stats = script_style(d)
    pipe = FramePipeline(net, lambda z, i: cw.transfer_with_stats(z, s_stats), CH, CW, src_yuv=DEEP_IN, out_yuv=DEEP_IN)
    want = run(pipe, flats)
    assert one_process == b"".join(w.tobytes() for w in want) and len({w.tobytes() for w in want}) == CN


def test_script_shards_and_gpus_equal_one_process(clip, one_process, tmp_path):
    import video_transfer
    d, flats = clip
    for r in range(2):
        part = video_transfer.main(script_args(d, "--out_dir", str(tmp_path / "sh"), "--shard", "%d/2" % r))
        assert part == str(tmp_path / "sh" / "clip_s" / ("part_%d.yuv" % r))
    merged = merge_parts(str(tmp_path / "sh" / NAME), [str(tmp_path / "sh" / "clip_s" / ("part_%d.yuv" % r)) for r in range(2)], CN,
                         DEEP_IN.frame_bytes(CH, CW))
    assert open(merged, "rb").read() == one_process
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py")] + script_args(d, "--out_dir", str(tmp_path / "g2"),
                                                                                             "--gpus", "2"),
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(tmp_path / "g2" / NAME, "rb").read() == one_process


def test_script_8_bit_y4m_to_12_bit_444(clip, tmp_path):
    import video_transfer
    import yuv_ref
    from vstnet_amd.resize import img_resize_device
    from vstnet_amd.yuv import YuvSpec, rgb_to_yuv_host, yuv_to_rgb_u8
    d, _ = clip
    spec8 = YuvSpec("420mpeg2", "bt601", "limited")
    flats = [rgb_to_yuv_host(scene(CH, CW, 600 + i), spec8) for i in range(3)]
    yuv_ref.write_y4m(str(tmp_path / "c.y4m"), flats, CW, CH, "C420mpeg2")
    out = video_transfer.main(["--video", str(tmp_path / "c.y4m"), "--style", str(d / "s.png"), "--synthetic_weights", "--max_size",
                               "64", "--out_dir", str(tmp_path / "o"), "--out_pix_fmt", "yuv444p12le"])
    assert out == str(tmp_path / "o" / ("c_s_%dx%d_yuv444p12le.yuv" % (CW, CH)))
    spec = DeepYuvSpec("444", "bt601", "limited", 12)
    got = RawYuvClip(out, CW, CH, "yuv444p12le")
    assert len(got) == 3
    net, cw, s_stats = script_style(d)
    with torch.no_grad():
        for i, f in enumerate(flats):
            u8 = img_resize_device(yuv_to_rgb_u8(torch.from_numpy(f).cuda(), CH, CW, spec8), 64, 4)
            sty = net._inverse(cw.transfer_with_stats(net.forward_u8(u8[None]), s_stats))
            assert np.array_equal(got[i], rgb_f32_to_yuv16(sty, spec).cpu().numpy()), i


def test_script_auto_seg_reads_the_8_bit_twin(tmp_path):
    """a deep source with a segmenter: the label maps are those of the u8 side output fed as RGB frames"""
    import video_transfer
    W, H = 64, 48
    flats = [deep_frame(DEEP_IN, H, W, 700 + i) for i in range(3)]
    R.write_raw(str(tmp_path / "clip.yuv"), flats)
    Image.fromarray(scene(72, 104, 50)).save(tmp_path / "s.png")
    seg = ["--style", str(tmp_path / "s.png"), "--synthetic_weights", "--max_size", "64", "--auto_seg", "--synthetic_seg_weights",
           "--seg_variant", "b1", "--no_seg_remap", "--save_seg_label"]
    video_transfer.main(["--video", str(tmp_path / "clip.yuv"), "--pix_fmt", "yuv420p10le", "--video_size", "%dx%d" % (W, H),
                         "--out_dir", str(tmp_path / "deep")] + seg)
    os.makedirs(tmp_path / "frames")
    for i, f in enumerate(flats):
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        yuv16_to_rgb_f32(torch.from_numpy(f).cuda(), H, W, DEEP_IN, out_u8=u8)
        Image.fromarray(u8.cpu().numpy()).save(tmp_path / "frames" / ("%03d.png" % i))
    video_transfer.main(["--video", str(tmp_path / "frames"), "--frames_only", "--out_dir", str(tmp_path / "rgb")] + seg)
    for i in range(3):
        a = np.asarray(Image.open(tmp_path / "deep" / "segmentation" / ("%05d_label.png" % i)))
        b = np.asarray(Image.open(tmp_path / "rgb" / "segmentation" / ("%05d_label.png" % i)))
        assert a.shape == (H, W) and np.array_equal(a, b), i
