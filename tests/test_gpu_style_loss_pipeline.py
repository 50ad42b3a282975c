"""FramePipeline(style_loss=..., content_loss=...) on the card: the written bytes do not change, and every frame's values are
those of vstnet_amd.vgg.StyleLoss called by hand on the frame the sink received (and on the content), bit for bit - the same
kernels on the same inputs in fixed reduction orders, whatever ring slot and stream the frame had.  Under the stabiliser the
measured frame is the written one, not the decoder's."""
import numpy as np
import pytest
import torch

from test_gpu_flow_pipeline import PARAMS, moving_clip
from test_gpu_guided_pipeline import setup  # noqa: F401  (the fixture: a small synthetic-weight net and a transform)

pytestmark = pytest.mark.gpu

H, W, N = 32, 48, 6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def clip():
    return moving_clip(N, H, W)


@pytest.fixture(scope="module")
def meter():
    """one encoder on synthetic weights and a style of another size than the frames"""
    import vgg_ref as R
    from vstnet_amd.vgg import StyleLoss, VGGEncoder
    return StyleLoss(VGGEncoder("synthetic", "cuda:0"), dev(R.image_u8(25, 31, 3)))


@pytest.fixture(scope="module")
def plain(setup, clip):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    out = []
    FramePipeline(net, tf, H, W, depth=3).run(clip, lambda i, a: out.append(a.copy()))
    return out


@pytest.mark.parametrize("content", (False, True), ids=("loss_s", "loss_s+loss_c"))
@pytest.mark.parametrize("depth,streams", ((2, 1), (4, 3)))
def test_values_are_the_meter_by_hand_and_bytes_do_not_change(setup, clip, plain, meter, depth, streams, content):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    got = []
    pipe = FramePipeline(net, tf, H, W, depth=depth, compute_streams=streams, style_loss=meter, content_loss=content)
    assert pipe.run(clip, lambda i, a: got.append(a.copy())) == N
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    assert sorted(pipe.style) == list(range(N)) and len(pipe.style_meters) == depth
    by_hand = meter.clone()
    for i in range(N):
        want = by_hand(dev(got[i]), dev(clip[i]) if content else None).cpu().numpy()
        v = np.array(pipe.style[i])
        assert v.shape == ((2,) if content else (1,)) and np.isfinite(v).all() and (v > 0).all()
        assert v.tobytes() == want.tobytes(), (i, v, want)
    assert len({pipe.style[i] for i in range(N)}) == N               # (frames that all differ: a stale slot cannot hide)
    # a second run of the same pipeline starts afresh
    pipe.run(clip[:2], lambda i, a: None)
    assert sorted(pipe.style) == [0, 1]


def test_stabilised_frames_are_measured_as_written(setup, clip, plain, meter):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    got = []
    pipe = FramePipeline(net, tf, H, W, depth=3, temporal=True, flow="estimate", flow_params=PARAMS, stabilise=True,
                         style_loss=meter, content_loss=True)
    pipe.run(clip, lambda i, a: got.append(a.copy()))
    changed = [i for i in range(N) if not np.array_equal(got[i], plain[i])]
    assert changed, "the stabiliser changed no frame: the test shows nothing"
    by_hand = meter.clone()
    for i in range(N):
        want = by_hand(dev(got[i]), dev(clip[i])).cpu().numpy()
        assert np.array(pipe.style[i]).tobytes() == want.tobytes(), i
    i = changed[0]
    assert pipe.style[i][0] != float(by_hand(dev(plain[i])).cpu()[0])          # not the decoder's frame
    # the Lab step's route measures its own written frame
    got2 = []
    p2 = FramePipeline(net, tf, H, W, depth=2, preserve_luminance=True, style_loss=meter)
    p2.run(clip[:3], lambda i, a: got2.append(a.copy()))
    for i in range(3):
        assert not np.array_equal(got2[i], plain[i])
        assert p2.style[i] == (float(by_hand(dev(got2[i])).cpu()[0]),)


def test_off_adds_nothing_and_refusals(setup, meter):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.yuv import DeepYuvSpec
    net, tf = setup
    off = FramePipeline(net, tf, H, W, depth=2)
    assert off.style_meters is None and off.d_style is None and off.h_style is None and off.style == {}
    assert off.consumed_at == ("encoder",)
    assert FramePipeline(net, tf, H, W, depth=2, style_loss=meter).consumed_at == ("encoder",)
    assert FramePipeline(net, tf, H, W, depth=2, style_loss=meter, content_loss=True).consumed_at == ("decode",)
    with pytest.raises(ValueError, match="high-bit-depth out_yuv"):
        FramePipeline(net, tf, H, W, style_loss=meter, out_yuv=DeepYuvSpec("420mpeg2", "bt709", "limited", 10))
    with pytest.raises(ValueError, match="out_height, out_width"):
        FramePipeline(net, tf, H, W, style_loss=meter, content_loss=True, out_height=64, out_width=96, decode=lambda z: None)
    with pytest.raises(ValueError, match="goes with style_loss"):
        FramePipeline(net, tf, H, W, content_loss=True)
    # another written size is fine without the content loss
    FramePipeline(net, tf, H, W, style_loss=meter, out_height=64, out_width=96, decode=lambda z: None)


def test_video_script_csv_and_shards(tmp_path, capsys, clip):
    """style.csv of one process, of two shards joined, and the values by hand on the written frames"""
    import os
    from PIL import Image
    import vgg_ref as R
    import video_transfer
    from vstnet_amd import style_files as S
    from vstnet_amd.vgg import StyleLoss, VGGEncoder
    fd = tmp_path / "clip"
    fd.mkdir()
    for i, f in enumerate(clip[:5]):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
    style = R.image_u8(36, 44, 8)
    Image.fromarray(style).save(tmp_path / "s.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--max_size", "64", "--synthetic_weights", "--frames_only"]

    def run(name, extra):
        d = video_transfer.main(base + ["--out_dir", str(tmp_path / name)] + extra)
        return d, [np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d)) if f.endswith(".png")]
    d_plain, plain_frames = run("plain", [])
    assert not os.path.exists(os.path.join(d_plain, S.CSV_NAME)) and "style" not in video_transfer.LAST_RUN
    capsys.readouterr()
    flags = ["--style_loss", "--content_loss", "--synthetic_vgg_weights"]
    d_one, one = run("one", flags)
    text = capsys.readouterr().out
    assert "style loss (VGG-19 relu1_1..relu4_1, 5 frames)" in text and "loss_s mean" in text and "loss_c mean" in text
    assert len(one) == 5 and all(np.array_equal(a, b) for a, b in zip(plain_frames, one))
    rows = S.read_csv(os.path.join(d_one, S.CSV_NAME))
    assert sorted(rows) == list(range(5)) and video_transfer.LAST_RUN["style"] == rows
    meter = StyleLoss(VGGEncoder("synthetic", "cuda:0"), dev(style))
    for i in range(5):
        want = meter(dev(one[i]), dev(clip[i])).cpu().numpy()
        assert np.array(rows[i]).tobytes() == want.tobytes(), i
    d0, _ = run("sh", flags + ["--shard", "0/2"])
    d1, _ = run("sh", flags + ["--shard", "1/2"])
    assert d0 == d1 and not os.path.exists(os.path.join(d0, S.CSV_NAME))
    joined = S.join_parts([os.path.join(d0, S.part_name(1)), os.path.join(d0, S.part_name(0))], tmp_path / "joined.csv", 5)
    assert open(joined, "rb").read() == open(os.path.join(d_one, S.CSV_NAME), "rb").read()
    # loss_s alone: two cells per line
    d_s, _ = run("s", ["--style_loss", "--synthetic_vgg_weights"])
    assert all(len(v) == 1 and v[0] == rows[i][0] for i, v in S.read_csv(os.path.join(d_s, S.CSV_NAME)).items())


def test_image_script_prints_the_values(tmp_path, capsys, clip):
    from PIL import Image
    import vgg_ref as R
    import image_transfer
    from vstnet_amd.vgg import StyleLoss, VGGEncoder
    style = R.image_u8(36, 44, 8)
    Image.fromarray(clip[0]).save(tmp_path / "c.png")
    Image.fromarray(style).save(tmp_path / "s.png")
    base = ["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--max_size", "64", "--synthetic_weights"]
    plain_img = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "p")])))
    assert "style" not in image_transfer.LAST_RUN
    capsys.readouterr()
    got = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "a"), "--style_loss", "--content_loss",
                                                            "--synthetic_vgg_weights"])))
    text = capsys.readouterr().out
    assert np.array_equal(plain_img, got) and "style loss (VGG-19 relu1_1..relu4_1" in text
    values = image_transfer.LAST_RUN["style"]
    want = StyleLoss(VGGEncoder("synthetic", "cuda:0"), dev(style))(dev(got), dev(clip[0])).cpu().numpy()
    assert values["loss_s"] == want[0] and values["loss_c"] == want[1] and ("%.6e" % values["loss_s"]) in text


def test_a_redone_frame_is_measured_on_its_second_decode():
    """frame 3 has ten valid labels and is done again on the dense route when it retires: its values are those of the frame
    that is written, not of the first decode the packed route left"""
    from models.cWCT import cWCT
    import vgg_ref as R
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.vgg import StyleLoss, VGGEncoder
    from tests.test_gpu_luminance import _net, _style
    from tests.test_gpu_masks import clip_maps
    hh, ww = 64, 96
    src = moving_clip(6, hh, ww)
    net, cw = _net(), cWCT()
    sty, maps = clip_maps()
    maps = [maps[k] for k in (0, 1, 2, 3, 6, 0)]
    assert maps[0].shape == (hh, ww)
    with torch.no_grad():
        binding = cw.bind_style_labels(_style(net, 9, sty.shape), sty)

    def planned(z_c, ms, cap):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(hh, ww, 32, "cuda")
        return cw.transfer_with_plan(z_c, None, cw.plan_frame(ms.mask, binding, max_slots=cap, buffers=buf, flags=ms.flags))
    tf = lambda z, i, ms: planned(z, ms, 8)                                     # noqa: E731
    redo = lambda z, i, ms: planned(z, ms, 32)                                  # noqa: E731
    meter = StyleLoss(VGGEncoder("synthetic", "cuda:0"), dev(R.image_u8(25, 31, 3)))
    plain_frames, got = [], []
    FramePipeline(net, tf, hh, ww, redo=redo).run(src, lambda i, a: plain_frames.append(a.copy()), masks=maps)
    pipe = FramePipeline(net, tf, hh, ww, redo=redo, style_loss=meter, content_loss=True)
    pipe.run(src, lambda i, a: got.append(a.copy()), masks=maps)
    assert pipe.redo_count == 1 and all(np.array_equal(a, b) for a, b in zip(plain_frames, got))
    by_hand = meter.clone()
    for i in range(6):
        want = by_hand(dev(got[i]), dev(src[i])).cpu().numpy()
        assert np.array(pipe.style[i]).tobytes() == want.tobytes(), i
