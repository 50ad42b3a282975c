"""FramePipeline(upscale="guided") and video_transfer.py --upscale guided on the card: every frame that leaves the ring equals,
bit for bit, the sequential chain by hand - DeviceImgResize, forward_u8, the transform, net(z, forward=False), GuidedUpscale -, so a
ring slot handed to its next tenant too early would show up here; the constructor's errors; shards write one process's bytes."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

HS, WS, MAX_SIZE, H, W, DEPTH = 96, 160, 64, 36, 64, 3


def frames(n, seed=0):
    """n source frames that all differ: a moving ramp under noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:HS, 0:WS]
    out = []
    for i in range(n):
        ramp = np.stack([(x + 9 * i) % WS / WS, y / HS, (x + y + 5 * i) % (WS + HS) / (WS + HS)], 2)
        out.append(np.clip(255 * (0.7 * ramp + 0.3 * rng.random((HS, WS, 3))), 0, 255).astype(np.uint8))
    return out


@pytest.fixture(scope="module")
def setup():
    from models.cWCT import cWCT
    from vstnet_amd.synth import synthetic_frames
    from tests.test_gpu_parity import make_net
    net, _, _ = make_net("photo")
    cw = cWCT()
    style = (synthetic_frames(1, 48, 64, seed=7)[0].permute(1, 2, 0) * 255).byte()[None].cuda()
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(style))
    return net, (lambda z, i: cw.transfer_with_stats(z, stats))


def by_hand(net, tf, src_frames, lum=False, radius=4, eps=1e-3):
    """the sequential chain, one frame at a time on the current stream, fresh buffers per frame"""
    from vstnet_amd.color import luminance_transfer_u8
    from vstnet_amd.guided import GuidedUpscale
    from vstnet_amd.resize import DeviceImgResize
    dev = torch.device("cuda")
    out = []
    with torch.no_grad():
        for i, f in enumerate(src_frames):
            src = torch.from_numpy(f).cuda()
            rs = DeviceImgResize((HS, WS), MAX_SIZE, 4, dev)
            assert rs.size_wh == (W, H)
            d_in = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
            rs(src, d_in)
            sty = net(tf(net.forward_u8(d_in), i), forward=False)
            if lum:
                sty = luminance_transfer_u8(d_in, sty, out=sty, to_float=True)
            out.append(GuidedUpscale((H, W), (HS, WS), radius, eps, dev)(d_in, sty, src))
    torch.cuda.synchronize()
    return out


def make_pipe(net, tf, **kw):
    from vstnet_amd.pipeline import FramePipeline
    args = dict(depth=DEPTH, compute_streams=2, src_height=HS, src_width=WS, max_size=MAX_SIZE, down_scale=4, out_height=HS,
                out_width=WS, upscale="guided")
    args.update(kw)
    return FramePipeline(net, tf, H, W, **args)


def test_ring_reuse_equals_the_chain_by_hand(setup):
    net, tf = setup
    src = frames(2 * DEPTH + 1)
    want = by_hand(net, tf, src)
    got = []
    pipe = make_pipe(net, tf)
    assert pipe.run(src, lambda i, a: got.append(a.copy())) == len(src)
    assert len(got) == len(src)
    for i in range(len(src)):
        assert got[i].shape == (HS, WS, 3)
        assert np.array_equal(got[i], want[i][0].cpu().numpy()), i
    assert len({g.tobytes() for g in got}) == len(src)              # (frames that all differ: a stale slot cannot hide)
    # the radius and the ridge reach the kernels
    got2 = []
    make_pipe(net, tf, upscale_radius=2, upscale_eps=1e-2).run(src[:2], lambda i, a: got2.append(a.copy()))
    want2 = by_hand(net, tf, src[:2], radius=2, eps=1e-2)
    assert all(np.array_equal(got2[i], want2[i][0].cpu().numpy()) for i in range(2)) and not np.array_equal(got2[0], got[0])
    # without the keyword nothing is made
    from vstnet_amd.pipeline import FramePipeline
    plain = FramePipeline(net, tf, H, W, depth=DEPTH, src_height=HS, src_width=WS, max_size=MAX_SIZE)
    assert plain.upscalers is None and plain.d_up is None and plain.d_up_out is None


def test_luminance_and_y4m(setup):
    from vstnet_amd.yuv import YuvSpec, rgb_to_yuv_host, rgb_to_yuv_u8, yuv_to_rgb_u8
    net, tf = setup
    src = frames(2 * DEPTH + 1, seed=1)
    want = by_hand(net, tf, src, lum=True)
    got = []
    make_pipe(net, tf, preserve_luminance=True).run(src, lambda i, a: got.append(a.copy()))
    for i in range(len(src)):
        assert np.array_equal(got[i], want[i][0].cpu().numpy()), i
    # 8-bit planes in and out: the chain by hand on the frames the conversion gives, converted as any other frame
    spec = YuvSpec("420jpeg", "bt709", "limited")
    planes = [rgb_to_yuv_host(f.astype(np.float64), spec) for f in src]
    # (the pipeline is bit-identical to feeding it the frames yuv_to_rgb_u8 gives - the card's conversion, not the host's)
    rgb = [yuv_to_rgb_u8(torch.from_numpy(p).cuda(), HS, WS, spec).cpu().numpy() for p in planes]
    want = by_hand(net, tf, rgb)
    got = []
    make_pipe(net, tf, src_yuv=spec, out_yuv=spec).run(planes, lambda i, a: got.append(a.copy()))
    for i in range(len(src)):
        assert got[i].shape == (spec.frame_bytes(HS, WS),)
        assert np.array_equal(got[i], rgb_to_yuv_u8(want[i].contiguous(), spec).cpu().numpy()), i


def test_constructor_errors(setup):
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.yuv import DeepYuvSpec
    net, tf = setup
    deep = DeepYuvSpec("420mpeg2", "bt709", "limited", 10)
    with pytest.raises(ValueError, match="src_height"):             # no source frame on the card
        FramePipeline(net, tf, H, W, upscale="guided")
    with pytest.raises(ValueError, match="uint8 source"):           # a deep source, even one resized on the card
        make_pipe(net, tf, src_yuv=deep, src_deep_resize=True)
    with pytest.raises(ValueError, match="out_height, out_width"):  # the frame leaves at the source size
        make_pipe(net, tf, out_height=H, out_width=W)
    with pytest.raises(ValueError, match="out_height, out_width"):
        make_pipe(net, tf, out_height=None, out_width=None)
    with pytest.raises(ValueError, match="decode hook"):
        make_pipe(net, tf, decode=lambda z: net.inverse_u8(z))
    with pytest.raises(ValueError, match="high-bit-depth out_yuv"):
        make_pipe(net, tf, out_yuv=deep)
    with pytest.raises(ValueError, match="radius"):
        make_pipe(net, tf, upscale_radius=9)
    with pytest.raises(ValueError, match="eps"):
        make_pipe(net, tf, upscale_eps=0.0)
    with pytest.raises(ValueError, match="upscale must be"):
        make_pipe(net, tf, upscale="lanczos")


def test_image_script_writes_the_source_size(tmp_path):
    """image_transfer.py --upscale guided: the result has the source image's size and is the chain by hand - img_resize, encode,
    cWCT.transfer, net(z, forward=False), guided_fit + guided_apply on the source image - bit for bit"""
    import image_transfer
    from models.cWCT import cWCT
    from utils.utils import img_resize, to_tensor_u8
    from vstnet_amd.guided import guided_apply, guided_fit
    src, style = frames(1, seed=4)[0], frames(1, seed=5)[0][:48, :64].copy()
    Image.fromarray(src).save(tmp_path / "c.png")
    Image.fromarray(style).save(tmp_path / "s.png")
    base = ["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--max_size", str(MAX_SIZE),
            "--synthetic_weights"]
    got = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "g"), "--upscale", "guided",
                                                            "--upscale_radius", "2", "--upscale_eps", "1e-2"])))
    plain = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "p")])))
    assert got.shape == (HS, WS, 3) and plain.shape == (H, W, 3)
    net = image_transfer.build_network("photorealistic", None, True, torch.device("cuda"), None)
    cw = cWCT()
    content = img_resize(Image.fromarray(src), MAX_SIZE, down_scale=net.down_scale)
    with torch.no_grad():
        c_u8 = to_tensor_u8(content).cuda()
        z_cs = cw.transfer(net.forward_u8(c_u8), net.forward_u8(to_tensor_u8(Image.fromarray(style)).cuda()), None, None)
        want = guided_apply(guided_fit(c_u8, net(z_cs, forward=False), 2, 1e-2), torch.from_numpy(src).cuda())
    assert np.array_equal(got, want[0].cpu().numpy())


def test_shards_write_one_process_bytes(tmp_path):
    import video_transfer
    fd = tmp_path / "clip"
    fd.mkdir()
    for i, f in enumerate(frames(5, seed=2)):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
    Image.fromarray(frames(1, seed=3)[0][:48, :64].copy()).save(tmp_path / "s.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--max_size", str(MAX_SIZE), "--synthetic_weights",
            "--frames_only", "--resize", "device"]

    def run(name, extra):
        d = video_transfer.main(base + ["--out_dir", str(tmp_path / name)] + extra)
        return [np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))]
    one = run("one", ["--upscale", "guided"])
    parts = run("s0", ["--upscale", "guided", "--shard", "0/2"]) + run("s1", ["--upscale", "guided", "--shard", "1/2"])
    assert len(one) == len(parts) == 5
    for i in range(5):
        assert one[i].shape == (HS, WS, 3) and np.array_equal(one[i], parts[i]), i
    plain = run("plain", ["--upscale", "bicubic"])
    assert len(plain) == 5 and all(p.tobytes() != g.tobytes() for p, g in zip(plain, one))
