"""The device resize on the card (csrc/resize.hip, vstnet_amd/resize.py): the input side against Pillow byte for byte, the
output side against F.interpolate evaluated in float64 on the CPU, the frame pipeline fed unresized frames against the same
pipeline fed host-resized ones, and video_transfer.py --resize device against --resize host."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from tests import resize_ref as ref

pytestmark = pytest.mark.gpu
T = torch.from_numpy

# (source w, h) -> (w, h): the shapes the restatement is pinned on (test_resize_host.py) and an odd near-identity shrink
U8_SHAPES = [((1920, 1080), (1280, 720)), ((3840, 2160), (1280, 720)), ((641, 363), (640, 360)), ((97, 55), (96, 52)),
             ((300, 200), (452, 300)), ((500, 333), (1280, 852)), ((1283, 719), (1280, 716))]


def _pil(img, size_wh):
    return np.asarray(Image.fromarray(img).resize(size_wh, Image.BICUBIC))


@pytest.mark.parametrize("src_wh,dst_wh", U8_SHAPES)
def test_resize_u8_equals_pillow(src_wh, dst_wh):
    from vstnet_amd.resize import resize_u8
    img = ref.frame(src_wh[1], src_wh[0], seed=src_wh[0] + 1)
    got = resize_u8(T(img).cuda(), dst_wh).cpu().numpy()
    want = _pil(img, dst_wh)
    assert got.shape == want.shape
    assert int((got != want).sum()) == 0


def test_resize_u8_smooth_frame_single_passes_and_copy():
    from vstnet_amd.resize import resize_u8
    img = ref.frame(1080, 1920, seed=2, smooth=True)           # smooth: sums sit near the rounding boundary, nothing clips
    d = T(img).cuda()
    for wh in ((1280, 720), (1920, 720), (1280, 1080), (1918, 1079), (1920, 1080)):      # both, vertical only, horizontal only, odd, copy
        got = resize_u8(d, wh).cpu().numpy()
        assert int((got != _pil(img, wh)).sum()) == 0, wh
    small = ref.frame(55, 97, seed=4, smooth=True)
    assert np.array_equal(resize_u8(T(small).cuda(), (33, 7)).cpu().numpy(), _pil(small, (33, 7)))      # ksize 33 vertically, odd sizes


@pytest.mark.parametrize("src_wh,max_size", [((1920, 1080), 1280), ((3840, 2160), 1280), ((1283, 719), 1280), ((1000, 562), 1280)])
def test_img_resize_device_equals_img_resize(src_wh, max_size):
    from utils.utils import img_resize
    from vstnet_amd.resize import img_resize_device, DeviceImgResize, img_resize_steps
    img = ref.frame(src_wh[1], src_wh[0], seed=src_wh[1])
    want = np.asarray(img_resize(Image.fromarray(img), max_size, down_scale=4))
    assert len(img_resize_steps(src_wh, max_size, 4)) == (2 if max(src_wh) > max_size else 1)
    got = img_resize_device(T(img).cuda(), max_size, 4).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    # the preallocated form the pipeline uses, twice into the same buffers
    rs = DeviceImgResize((src_wh[1], src_wh[0]), max_size, 4, torch.device("cuda"))
    out = torch.empty((1, want.shape[0], want.shape[1], 3), dtype=torch.uint8, device="cuda")
    for _ in range(2):
        out.zero_()
        rs(T(img).cuda(), out)
        assert np.array_equal(out[0].cpu().numpy(), want)


F32_SHAPES = [((720, 1280), (1080, 1280)), ((360, 640), (1080, 1920)), ((716, 1280), (719, 1283)), ((256, 256), (100, 180))]


def _f32_case(src_hw, dst_hw, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((1, 3) + src_hw, generator=g) * 1.2 - 0.1               # [-0.1, 1.1]: both clamps are exercised
    v64 = F.interpolate(x.double(), size=dst_hw, mode="bicubic", align_corners=False, antialias=True)
    return x, v64


@pytest.mark.parametrize("src_hw,dst_hw", F32_SHAPES)
def test_resize_f32_against_float64(src_hw, dst_hw):
    """Bound 1e-5: two passes of at most ksize + 2 fp32 roundings on values of magnitude <= 1.1 with sum |w| <= ~1.4 per pass,
    about 2e-6 at the largest ksize here, with a 5x margin.  The stock fp32 resize's own deviation from the same oracle is
    printed next to it (5e-5 to 1.4e-4: its coordinates and weights are computed in fp32)."""
    from vstnet_amd.resize import resize_f32
    x, v64 = _f32_case(src_hw, dst_hw, seed=src_hw[0])
    got = resize_f32(x.cuda(), dst_hw).cpu()
    assert got.shape == v64.shape and got.dtype == torch.float32
    err = float((got.double() - v64).abs().max())
    stock = float((F.interpolate(x, size=dst_hw, mode="bicubic", align_corners=False, antialias=True).double() - v64).abs().max())
    print(f"resize_f32 {src_hw}->{dst_hw}: max abs error {err:.3e} (stock fp32 resize on the CPU: {stock:.3e})")
    assert err <= 1e-5


@pytest.mark.parametrize("src_hw,dst_hw", F32_SHAPES)
def test_resize_to_u8_against_float64(src_hw, dst_hw):
    """A byte may differ from the quantised float64 result by 1, and only where 255 * v64 lies within 2.55e-3 (= 255 * 1e-5) of
    an integer; such bytes are at most 1 % of the frame (the oracle alone puts 0.43-0.48 % of them that close)."""
    from vstnet_amd.resize import resize_to_u8
    x, v64 = _f32_case(src_hw, dst_hw, seed=src_hw[1] + 1)
    got = resize_to_u8(x.cuda(), dst_hw).cpu()
    assert got.shape == (1,) + dst_hw + (3,) and got.dtype == torch.uint8
    s = v64.mul(255).permute(0, 2, 3, 1)
    want = s.clamp(0, 255).byte()
    near = (s - s.round()).abs() <= 2.55e-3
    d = (got.int() - want.int()).abs()
    print(f"resize_to_u8 {src_hw}->{dst_hw}: {int((d > 0).sum())} bytes differ (max {int(d.max())}), "
          f"{float(near.float().mean()):.4%} of the oracle's values are within 2.55e-3 of an integer")
    assert int(d.max()) <= 1
    assert not bool(((d > 0) & ~near).any())
    assert float(((d > 0) & near).float().mean()) <= 0.01
    # several images in one call: the planes of image b, the rows of image b
    xb = torch.cat([x, x.flip(3), x * 0.5], 0)
    gb = resize_to_u8(xb.cuda(), dst_hw).cpu()
    assert torch.equal(gb[0], got[0])
    vb = F.interpolate(xb[2:].double(), size=dst_hw, mode="bicubic", align_corners=False, antialias=True).mul(255)
    assert int((gb[2].int() - vb.permute(0, 2, 3, 1)[0].clamp(0, 255).byte().int()).abs().max()) <= 1


def test_frame_pipeline_resizes_on_the_device():
    """FramePipeline(src_height, src_width) fed decoded frames against the same pipeline fed host-resized frames: the inputs
    of the net are the same bytes (tests above), so the stylised uint8 frames are the same bytes."""
    from models.cWCT import cWCT
    from utils.utils import img_resize
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_frames
    from tests.test_gpu_parity import make_net
    net, _, _ = make_net("photo")
    cw = cWCT()
    Hs, Ws, max_size, N = 217, 387, 256, 7
    frames = [ref.frame(Hs, Ws, seed=40 + i, smooth=bool(i & 1)) for i in range(N)]
    resized = [np.asarray(img_resize(Image.fromarray(f), max_size, down_scale=4)) for f in frames]
    H, W = resized[0].shape[:2]
    assert (W, H) == (256, 140)
    style = (synthetic_frames(1, 48, 64, seed=7)[0].permute(1, 2, 0) * 255).byte()[None].cuda()
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(style))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)      # noqa: E731
    want, got = [], []
    FramePipeline(net, tf, H, W, depth=3, compute_streams=2).run(resized, lambda i, a: want.append(a.copy()))
    pipe = FramePipeline(net, tf, H, W, depth=3, compute_streams=2, src_height=Hs, src_width=Ws, max_size=max_size, down_scale=4)
    assert pipe.run(frames, lambda i, a: got.append(a.copy())) == N
    assert len(got) == len(want) == N
    for i in range(N):
        assert np.array_equal(got[i], want[i]), i
    with pytest.raises(ValueError):
        pipe.run([resized[0]], lambda i, a: None)              # this pipeline takes source-size frames
    with pytest.raises(ValueError):
        FramePipeline(net, tf, H, W + 4, src_height=Hs, src_width=Ws, max_size=max_size)


def _bands(h, w, labels):
    m = np.zeros((h, w), np.uint8)
    edges = np.linspace(0, w, len(labels) + 1).astype(int)
    for k, l in enumerate(labels):
        m[:, edges[k]:edges[k + 1]] = l
    return m


def _read(d):
    return [np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))]


def _close(a, b, what):
    d = np.abs(a.astype(int) - b.astype(int))
    print(f"{what}: max diff {d.max()}, differing {(d > 0).mean():.3%}, mean abs {d.mean():.2e}")
    assert d.max() <= 1 and (d > 0).mean() <= 0.01 and d.mean() < 0.01, what


def test_video_transfer_device_resize_against_host(tmp_path):
    """An 8-frame 192x108 clip at --max_size 128 (stylised at 128x72, written at 128x108): every frame of --resize device is
    within one count of --resize host on at most 1 % of its bytes (the stock fp32 resize is itself that far from exact); a shard
    of the device run and the masked device run's shard give the unsharded run's frames bit for bit."""
    import video_transfer
    fd, sd_ = tmp_path / "clip", tmp_path / "segs"
    fd.mkdir()
    sd_.mkdir()
    for i in range(8):
        Image.fromarray(ref.frame(108, 192, seed=60 + i, smooth=True)).save(fd / f"{i:03d}.png")
        Image.fromarray(_bands(108, 192, [0, 1, 2] if i & 1 else [1, 0]), mode="L").save(sd_ / f"{i:03d}.png")
    Image.fromarray(ref.frame(96, 128, seed=5, smooth=True)).save(tmp_path / "s.png")
    Image.fromarray(_bands(96, 128, [0, 1, 2]), mode="L").save(tmp_path / "sseg.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--max_size", "128", "--synthetic_weights", "--frames_only"]
    masks = ["--content_seg_dir", str(sd_), "--style_seg", str(tmp_path / "sseg.png")]

    def run(name, extra):
        return _read(video_transfer.main(base + ["--out_dir", str(tmp_path / name)] + extra))

    host = run("host", ["--resize", "host"])
    dev = run("dev", ["--resize", "device"])
    assert len(host) == len(dev) == 8
    for i in range(8):
        assert dev[i].shape == (108, 128, 3)
        _close(dev[i], host[i], f"frame {i}")
    shard = run("shard", ["--resize", "device", "--shard", "1/2"])
    assert len(shard) == 4
    for i in range(4):
        assert np.array_equal(shard[i], dev[4 + i]), i
    mdev = run("mdev", ["--resize", "device"] + masks)
    mhost = run("mhost", ["--resize", "host"] + masks)
    for i in range(8):
        _close(mdev[i], mhost[i], f"masked frame {i}")
    mshard = run("mshard", ["--resize", "device", "--shard", "1/2"] + masks)
    assert len(mshard) == 4
    for i in range(4):
        assert np.array_equal(mshard[i], mdev[4 + i]), i
