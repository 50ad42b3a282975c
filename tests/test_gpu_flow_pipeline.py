"""FramePipeline(temporal=True, flow="estimate") and video_transfer.py --temporal --estimate_flow on the card: the written bytes do
not change, and every frame's values are those of vstnet_amd.flow.estimate_flow, consistency and temporal.temporal_loss called by
hand on the frames the sink received and on the inputs the test holds - bit for bit: the same kernels on the same inputs, whatever
ring slot and stream the frame and its predecessor had (an estimator workspace or a history slot handed on too early would show
up here)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import flow_ref as R
from test_gpu_guided_pipeline import setup  # noqa: F401  (the fixture: a small synthetic-weight net and a transform)

pytestmark = pytest.mark.gpu

H, W, N = 64, 96, 6
PARAMS = dict(levels=3, iters=2, radius=2, lam=2e-3)


def moving_clip(n=N, h=H, w=W):
    """n uint8 frames: one texture drifting by (1.5, -0.7) px per frame, with a growing smooth deformation"""
    tex = R.texture(h, w, 9)
    bend = R.smooth_flow(h, w, 0.4, (1.5, -0.7), 9)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return [R.to_u8(np.stack([R.bilinear(np.ascontiguousarray(tex[..., c]), yy - t * bend[1], xx - t * bend[0]) for c in range(3)], -1))
            for t in range(n)]


@pytest.fixture(scope="module")
def clip():
    return moving_clip()


@pytest.fixture(scope="module")
def plain(setup, clip):  # noqa: F811
    """the same frames through a pipeline without the flags: computed once"""
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    out = []
    FramePipeline(net, tf, H, W, depth=3).run(clip, lambda i, a: out.append(a.copy()))
    return out


def by_hand(prev_in, cur_in, prev_out, cur_out, mask, params):
    """(loss_out, loss_in[, share]) of one frame pair from the library calls"""
    from vstnet_amd.flow import consistency, estimate_flow
    from vstnet_amd.temporal import mean3, temporal_loss
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    prev_in, cur_in, prev_out, cur_out = d(prev_in), d(cur_in), d(prev_out), d(cur_out)
    flow = estimate_flow(cur_in, prev_in, **params)
    valid = consistency(flow, estimate_flow(prev_in, cur_in, **params)) if mask else None
    lo = temporal_loss(prev_out, cur_out, flow, valid=valid).cpu().numpy()
    li = temporal_loss(prev_in, cur_in, flow, valid=valid).cpu().numpy()
    row = (mean3(lo[:3]), mean3(li[:3]))
    return row + (float(li[3]),) if mask else row


@pytest.mark.parametrize("depth,streams", ((2, 1), (4, 3)))
@pytest.mark.parametrize("mask", (False, True))
def test_values_by_hand_and_same_bytes(setup, clip, plain, depth, streams, mask):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    pipe = FramePipeline(net, tf, H, W, depth=depth, compute_streams=streams, temporal=True, flow="estimate", flow_mask=mask,
                         flow_params=PARAMS)
    got = []
    assert pipe.run(clip, lambda i, a: got.append(a.copy())) == N
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    assert sorted(pipe.temporal) == list(range(1, N))               # frame 0 has no value
    for i in range(1, N):
        want = by_hand(clip[i - 1], clip[i], got[i - 1], got[i], mask, PARAMS)
        assert pipe.temporal[i] == want and len(want) == (3 if mask else 2), (i, pipe.temporal[i], want)
        assert all(isinstance(v, float) for v in want) and want[0] > 0.0 and want[1] > 0.0
        if mask:
            assert 0.5 < want[2] < 1.0              # (the frame's border moves out of sight: never everything)
    assert len({pipe.temporal[i] for i in range(1, N)}) == N - 1    # (pairs that all differ: a stale slot cannot hide)
    # the estimated flow does what it is for: the input pair's warping error is well below its plain frame difference
    from vstnet_amd.temporal import mean3, temporal_loss
    d = lambda a: torch.from_numpy(a).cuda()                            # noqa: E731
    plain_diff = mean3(temporal_loss(d(clip[2]), d(clip[3]), None).cpu().numpy())
    assert pipe.temporal[3][1] < 0.5 * plain_diff, (pipe.temporal[3], plain_diff)


def test_off_makes_nothing_and_errors(setup):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    on = FramePipeline(net, tf, H, W, temporal=True)
    assert on.t_estimators is None and on.t_flow_h is not None and tuple(on.d_temporal.shape) == (on.depth, 2, 3)
    est = FramePipeline(net, tf, H, W, temporal=True, flow="estimate")
    assert est.t_flow_h is None and est.t_estimators[0].valid is None and tuple(est.d_temporal.shape) == (est.depth, 2, 3)
    with pytest.raises(ValueError, match="flow='estimate'"):
        est.run([], lambda i, a: None, flows=[])
    with pytest.raises(ValueError, match="temporal=True"):
        FramePipeline(net, tf, H, W, flow="estimate")
    with pytest.raises(ValueError, match="flow='estimate'"):
        FramePipeline(net, tf, H, W, temporal=True, flow_mask=True)
    with pytest.raises(ValueError, match="flow must be"):
        FramePipeline(net, tf, H, W, temporal=True, flow="farneback")


@pytest.mark.parametrize("mask", (False, True))
def test_video_script_estimate_flow(tmp_path, capsys, clip, mask):
    import video_transfer
    from vstnet_amd import flowfiles as FF
    fd = tmp_path / "clip"
    fd.mkdir()
    n = 4
    for t in range(n):
        Image.fromarray(clip[t]).save(fd / f"{t:03d}.png")
    Image.fromarray(R.to_u8(R.texture(48, 64, 4))).save(tmp_path / "s.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--max_size", "96", "--synthetic_weights", "--frames_only"]
    d0 = video_transfer.main(base + ["--out_dir", str(tmp_path / "plain")])
    capsys.readouterr()
    flags = ["--temporal", "--estimate_flow", "--flow_levels", "3", "--flow_iters", "2", "--flow_radius", "2", "--flow_lambda", "2e-3"]
    d = video_transfer.main(base + ["--out_dir", str(tmp_path / "o")] + flags + (["--flow_mask"] if mask else []))
    text = capsys.readouterr().out
    assert "temporal (warping error, 3 frame pairs)" in text and ("mean valid share" in text) == mask
    names = sorted(f for f in os.listdir(d) if f.endswith(".png"))
    assert len(names) == n and names == sorted(f for f in os.listdir(d0) if f.endswith(".png"))
    for f in names:                                 # the frames are those of the run without --temporal, byte for byte
        assert open(os.path.join(d, f), "rb").read() == open(os.path.join(d0, f), "rb").read()
    written = [np.asarray(Image.open(os.path.join(d, f))).copy() for f in names]
    lines = open(os.path.join(d, FF.CSV_NAME)).read().splitlines()
    assert len(lines) == n and lines[0] == ("0,,," if mask else "0,,")
    rows = FF.read_csv(os.path.join(d, FF.CSV_NAME))
    for t in range(1, n):
        want = by_hand(clip[t - 1], clip[t], written[t - 1], written[t], mask, PARAMS)
        assert rows[t] == want == video_transfer.LAST_RUN["temporal"][t], (t, rows[t], want)
        assert lines[t] == ",".join(["%d" % t] + ["%r" % v for v in want])
