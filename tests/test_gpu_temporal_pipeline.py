"""FramePipeline(temporal=True) and video_transfer.py --temporal on the card: the written bytes do not change, every frame's two
values are those of vstnet_amd.temporal.temporal_loss called by hand on the frames the sink received and on the clip's own frames
(bit for bit: the same kernels on the same inputs, whatever ring slot and stream the frame and its predecessor had - a history slot
handed to its next tenant too early would show up here), the first frame has no value, and the script's temporal.csv holds the
library's numbers."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import temporal_ref as R
from test_gpu_guided_pipeline import setup  # noqa: F401  (the fixture: a small synthetic-weight net and a transform)

pytestmark = pytest.mark.gpu

H, W, N = 64, 96, 6


@pytest.fixture(scope="module")
def clip():
    from vstnet_amd.temporal import synthetic_clip
    frames, flows, loss_in = synthetic_clip(R.make_frame_u8(H, W), N, seed=1, cell=16, ksize=16)
    torch.cuda.synchronize()
    return frames, flows, loss_in.cpu().numpy()


@pytest.fixture(scope="module")
def plain(setup, clip):  # noqa: F811
    """the same frames through a pipeline without the flag: computed once"""
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    out = []
    FramePipeline(net, tf, H, W, depth=3).run(list(clip[0].cpu().numpy()), lambda i, a: out.append(a.copy()))
    return out


@pytest.mark.parametrize("depth,streams", ((2, 1), (2, 3), (4, 1), (4, 3)))
def test_values_by_hand_and_same_bytes(setup, clip, plain, depth, streams):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.temporal import mean3, temporal_loss
    net, tf = setup
    frames, flows, loss_in = clip
    src = list(frames.cpu().numpy())
    pipe = FramePipeline(net, tf, H, W, depth=depth, compute_streams=streams, temporal=True)
    got = []
    # every other flow from the host, the rest as device tensors
    entries = [None] + [flows[t] if t % 2 else flows[t].cpu().numpy() for t in range(1, N)]
    assert pipe.run(src, lambda i, a: got.append(a.copy()), flows=entries) == N
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    assert sorted(pipe.temporal) == list(range(1, N))               # frame 0 has no value
    for i in range(1, N):
        lo, li = pipe.temporal[i]
        want_out = mean3(temporal_loss(torch.from_numpy(got[i - 1]).cuda(), torch.from_numpy(got[i]).cuda(), flows[i]).cpu().numpy())
        want_in = mean3(temporal_loss(frames[i - 1], frames[i], flows[i]).cpu().numpy())
        assert isinstance(lo, float) and lo == want_out and lo > 0.0, (i, lo, want_out)
        assert li == want_in and li == loss_in[i], (i, li, want_in, loss_in[i])
    assert len({pipe.temporal[i] for i in range(1, N)}) == N - 1    # (pairs that all differ: a stale slot cannot hide)
    # a second run starts a new history; a frame without a flow has no value and is still its successor's predecessor
    got2 = []
    pipe.run(src[2:5], lambda i, a: got2.append(a.copy()), start_index=2, flows=[flows[2], None, flows[4]])
    assert sorted(pipe.temporal) == [4] and pipe.temporal[4][1] == loss_in[4]


def test_a_redone_frame_has_a_stale_history(clip):
    """frame 3 has ten valid labels and is done again on the dense route when it retires: the history holds its first decode,
    so its own loss_out and its successor's are nan; loss_in and every other frame are untouched, as are the written bytes"""
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.temporal import mean3, temporal_loss
    from tests.test_gpu_luminance import _net, _style
    from tests.test_gpu_masks import clip_maps
    frames, flows, loss_in = clip
    src = list(frames.cpu().numpy())
    net, cw = _net(), cWCT()
    sty, maps = clip_maps()
    maps = [maps[k] for k in (0, 1, 2, 3, 6, 0)]
    assert maps[0].shape == (H, W) and len(maps) == N
    with torch.no_grad():
        binding = cw.bind_style_labels(_style(net, 9, sty.shape), sty)

    def planned(z_c, ms, cap):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, "cuda")
        return cw.transfer_with_plan(z_c, None, cw.plan_frame(ms.mask, binding, max_slots=cap, buffers=buf, flags=ms.flags))
    tf = lambda z, i, ms: planned(z, ms, 8)                                     # noqa: E731
    redo = lambda z, i, ms: planned(z, ms, 32)                                  # noqa: E731
    plain, got = [], []
    FramePipeline(net, tf, H, W, redo=redo).run(src, lambda i, a: plain.append(a.copy()), masks=maps)
    pipe = FramePipeline(net, tf, H, W, redo=redo, temporal=True)
    pipe.run(src, lambda i, a: got.append(a.copy()), masks=maps, flows=[None] + [flows[t] for t in range(1, N)])
    assert pipe.redo_count == 1 and all(np.array_equal(a, b) for a, b in zip(plain, got))
    assert sorted(pipe.temporal) == list(range(1, N))
    for i in range(1, N):
        lo, li = pipe.temporal[i]
        assert li == loss_in[i]
        if i in (3, 4):
            assert np.isnan(lo)
        else:
            assert lo == mean3(temporal_loss(torch.from_numpy(got[i - 1]).cuda(), torch.from_numpy(got[i]).cuda(), flows[i]).cpu().numpy())


def test_off_makes_nothing_and_errors(setup):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.yuv import DeepYuvSpec
    net, tf = setup
    off = FramePipeline(net, tf, H, W)
    assert off.t_in is None and off.t_flow is None and off.d_temporal is None and off.temporal == {}
    with pytest.raises(ValueError, match="temporal=True"):
        off.run([], lambda i, a: None, flows=[])
    with pytest.raises(ValueError, match="high-bit-depth out_yuv"):
        FramePipeline(net, tf, H, W, temporal=True, out_yuv=DeepYuvSpec("420mpeg2", "bt709", "limited", 10))
    with pytest.raises(ValueError, match="out_height, out_width"):
        FramePipeline(net, tf, H, W, temporal=True, out_height=2 * H, out_width=2 * W, decode=lambda z: None)
    with pytest.raises(ValueError, match="upscale='guided'"):
        FramePipeline(net, tf, 36, 64, temporal=True, src_height=96, src_width=160, max_size=64, out_height=96, out_width=160,
                      upscale="guided")
    on = FramePipeline(net, tf, H, W, temporal=True)
    with pytest.raises(ValueError, match="temporal=True"):
        on.run([], lambda i, a: None)
    with pytest.raises(ValueError, match="flow must be float32"):
        on.run([R.make_frame_u8(H, W)], lambda i, a: None, flows=[np.zeros((2, H, W + 1), np.float32)])


def test_video_script_synthetic_motion(tmp_path, capsys):
    import video_transfer
    from vstnet_amd import flowfiles as FF
    from vstnet_amd.temporal import mean3, temporal_loss
    Image.fromarray(R.make_frame_u8(H, W, 3)).save(tmp_path / "still.png")
    Image.fromarray(R.make_frame_u8(48, 64, 4)).save(tmp_path / "s.png")
    base = ["--video", str(tmp_path / "still.png"), "--style", str(tmp_path / "s.png"), "--max_size", "96", "--synthetic_weights",
            "--frames_only", "--out_dir", str(tmp_path / "o")]
    d = video_transfer.main(base + ["--temporal", "--synthetic_motion", "4", "--motion_seed", "2"])
    text = capsys.readouterr().out
    assert "temporal (warping error, 3 frame pairs)" in text and "amplification" in text
    lines = open(os.path.join(d, FF.CSV_NAME)).read().splitlines()
    assert len(lines) == 4 and lines[0] == "0,,"
    rows = FF.read_csv(os.path.join(d, FF.CSV_NAME))
    syn = video_transfer.LAST_RUN["synthetic"]
    written = [torch.from_numpy(np.asarray(Image.open(os.path.join(d, f))).copy()).cuda()
               for f in sorted(os.listdir(d)) if f.endswith(".png")]
    assert len(written) == 4
    for t in range(1, 4):
        want_out = mean3(temporal_loss(written[t - 1], written[t], syn["flows"][t]).cpu().numpy())
        assert rows[t] == (want_out, float(syn["loss_in"][t])) == video_transfer.LAST_RUN["temporal"][t]
        assert lines[t] == "%d,%r,%r" % (t, rows[t][0], rows[t][1])
    # the same clip from files: the frames as PNGs, the flows as .flo, give the same numbers
    fd, fl = tmp_path / "clip", tmp_path / "flows"
    fd.mkdir()
    fl.mkdir()
    for t, f in enumerate(syn["frames"].cpu().numpy()):
        Image.fromarray(f).save(fd / f"{t:03d}.png")
    for t in range(1, 4):
        FF.write_flo(fl / f"{t - 1:03d}.flo", syn["flows"][t].cpu().numpy())
    d2 = video_transfer.main(["--video", str(fd)] + base[2:-1] + [str(tmp_path / "o2"), "--temporal", "--flow_dir", str(fl)])
    assert FF.read_csv(os.path.join(d2, FF.CSV_NAME)) == rows
