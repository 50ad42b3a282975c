"""FramePipeline(temporal=True, stabilise=...) and video_transfer.py --temporal --stabilise on the card: the written frames are those
of a recursion done by hand - from the frames a run without the flag writes, the clip, the flows (given, or estimate_flow /
consistency called directly) and the numpy statement of the blend (tests/stabilise_ref.py) - byte for byte, whatever ring slot and
stream a frame and its predecessor had: a blend that ran ahead of its predecessor's, a history plane handed on too early or a later
step that read the decoder's frame instead of the written one would show up here.  The values are those of the meter called by
hand on the written and on the plain pairs."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import flow_ref as R
import stabilise_ref as S
from test_gpu_flow_pipeline import H, W, N, PARAMS, moving_clip
from test_gpu_guided_pipeline import setup  # noqa: F401  (the fixture: a small synthetic-weight net and a transform)

pytestmark = pytest.mark.gpu

STAB = dict(gain=0.6, sigma=12.0, limit=20.0)
NO_FLOW = 3                                         # source "given": this frame comes without a flow


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


@pytest.fixture(scope="module")
def by_hand(clip, plain):
    """source -> (flows, valids, written frames, {i: (loss_out, loss_in[, share])}, {i: loss_raw}): made once per source"""
    from vstnet_amd.flow import consistency, estimate_flow
    from vstnet_amd.temporal import mean3, temporal_loss
    made = {}

    def make(source):
        if source in made:
            return made[source]
        mask = source == "estimate_mask"
        flows, valids = [None] * N, [None] * N
        for t in range(1, N):
            if source == "given":
                if t != NO_FLOW:
                    flows[t] = R.smooth_flow(H, W, 0.5, (1.5 - 0.2 * t, -0.7), t).astype(np.float32)
            else:
                f = estimate_flow(dev(clip[t]), dev(clip[t - 1]), **PARAMS)
                flows[t] = f.cpu().numpy()
                if mask:
                    valids[t] = consistency(f, estimate_flow(dev(clip[t - 1]), dev(clip[t]), **PARAMS)).cpu().numpy()
        written = S.run_sequence(clip, plain, flows, valids, **STAB)
        values, raw = {}, {}
        for t in range(1, N):
            if flows[t] is None:
                continue
            v = None if valids[t] is None else dev(valids[t])
            lo = temporal_loss(dev(written[t - 1]), dev(written[t]), dev(flows[t]), valid=v).cpu().numpy()
            li = temporal_loss(dev(clip[t - 1]), dev(clip[t]), dev(flows[t]), valid=v).cpu().numpy()
            lr = temporal_loss(dev(plain[t - 1]), dev(plain[t]), dev(flows[t]), valid=v).cpu().numpy()
            values[t] = (mean3(lo[:3]), mean3(li[:3])) + ((float(li[3]),) if mask else ())
            raw[t] = mean3(lr[:3])
        made[source] = (flows, valids, written, values, raw)
        return made[source]
    return make


@pytest.mark.parametrize("depth,streams", ((2, 1), (4, 3)))
@pytest.mark.parametrize("source", ("given", "estimate", "estimate_mask"))
def test_written_frames_are_the_recursion_by_hand(setup, clip, plain, by_hand, depth, streams, source):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    flows, valids, written, values, raw = by_hand(source)
    kw = dict(flow="estimate", flow_mask=source == "estimate_mask", flow_params=PARAMS) if source != "given" else {}
    pipe = FramePipeline(net, tf, H, W, depth=depth, compute_streams=streams, temporal=True, stabilise=STAB, **kw)
    assert tuple(pipe.t_written.shape) == (depth, H, W, 3) and len(pipe.t_blended) == depth
    assert tuple(pipe.d_temporal.shape) == (depth, 3, 4 if source == "estimate_mask" else 3)
    got = []
    run_kw = dict(flows=[None if f is None else dev(f) for f in flows]) if source == "given" else {}
    assert pipe.run(clip, lambda i, a: got.append(a.copy()), **run_kw) == N
    for t in range(N):
        assert np.array_equal(got[t], written[t]), (t, int((got[t] != written[t]).sum()))
    assert np.array_equal(got[0], plain[0])
    if source == "given":                           # a frame without a flow is written as it is, and the recursion goes on from it
        assert np.array_equal(got[NO_FLOW], plain[NO_FLOW])
    live = [t for t in range(1, N) if flows[t] is not None]
    assert all((got[t] != plain[t]).mean() > 0.05 for t in live)     # (the blend changes the frames: the comparison means something)
    assert sorted(pipe.temporal) == live == sorted(pipe.stabilised)
    for t in live:
        assert pipe.temporal[t] == values[t], (t, pipe.temporal[t], values[t])
        assert pipe.stabilised[t] == raw[t], (t, pipe.stabilised[t], raw[t])
        assert isinstance(pipe.stabilised[t], float) and raw[t] > 0.0 and values[t][0] != raw[t]
    # a second run of the same object starts a new history
    got2 = []
    pipe.run(clip[:3], lambda i, a: got2.append(a.copy()), **(dict(flows=run_kw["flows"][:3]) if run_kw else {}))
    assert all(np.array_equal(a, b) for a, b in zip(got2, written[:3])) and sorted(pipe.stabilised) == [1, 2]


def test_flag_off_writes_the_plain_bytes(setup, clip, plain):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    for stab in (None, False):
        pipe = FramePipeline(net, tf, H, W, depth=3, temporal=True, flow="estimate", flow_params=PARAMS, stabilise=stab)
        assert pipe.t_written is None and pipe.t_blended is None and pipe.stab_params is None
        assert tuple(pipe.d_temporal.shape) == (3, 2, 3)
        got = []
        pipe.run(clip, lambda i, a: got.append(a.copy()))
        assert all(np.array_equal(a, b) for a, b in zip(plain, got))
        assert pipe.stabilised == {} and sorted(pipe.temporal) == list(range(1, N))
    off = FramePipeline(net, tf, H, W)
    assert off.stabilised == {} and off.stab_params is None and off.t_written is None


def test_constructor_errors(setup):  # noqa: F811
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    with pytest.raises(ValueError, match="temporal=True"):
        FramePipeline(net, tf, H, W, stabilise=True)
    with pytest.raises(ValueError, match="temporal=True"):
        FramePipeline(net, tf, H, W, stabilise=dict(gain=0.5))
    with pytest.raises(ValueError, match="mask slots"):
        FramePipeline(net, tf, H, W, temporal=True, stabilise=True, segmenter=object())
    for bad in (dict(gain=0.0), dict(gain=1.0), dict(sigma=0.0), dict(limit=-1.0), dict(strength=1.0)):
        with pytest.raises(ValueError):
            FramePipeline(net, tf, H, W, temporal=True, stabilise=bad)
    with pytest.raises(ValueError, match="None, True or a dict"):
        FramePipeline(net, tf, H, W, temporal=True, stabilise=0.7)
    # what temporal refuses stays refused
    with pytest.raises(ValueError, match="out_height"):
        FramePipeline(net, tf, H, W, temporal=True, stabilise=True, out_height=H + 4, out_width=W,
                      decode=lambda z: None)
    on = FramePipeline(net, tf, H, W, temporal=True, stabilise=True)
    assert on.stab_params == S.DEFAULTS
    with pytest.raises(ValueError, match="mask slots"):
        on.run([], lambda i, a: None, flows=[], masks=[])


def test_video_script_stabilise(tmp_path, capsys):
    import temporal_ref as T
    import video_transfer
    from vstnet_amd import flowfiles as FF
    from vstnet_amd.temporal import mean3, temporal_loss
    Image.fromarray(T.make_frame_u8(H, W, 3)).save(tmp_path / "still.png")
    Image.fromarray(T.make_frame_u8(48, 64, 4)).save(tmp_path / "s.png")
    base = ["--video", str(tmp_path / "still.png"), "--style", str(tmp_path / "s.png"), "--max_size", "96", "--synthetic_weights",
            "--frames_only", "--temporal", "--synthetic_motion", "5", "--motion_seed", "2"]
    d0 = video_transfer.main(base + ["--out_dir", str(tmp_path / "plain")])
    plain_rows = dict(video_transfer.LAST_RUN["temporal"])
    assert "stabilised" not in video_transfer.LAST_RUN and not os.path.exists(os.path.join(d0, FF.STABILISE_CSV_NAME))
    capsys.readouterr()
    d = video_transfer.main(base + ["--out_dir", str(tmp_path / "o"), "--stabilise"])
    text = capsys.readouterr().out
    assert "temporal (warping error, 4 frame pairs)" in text and "stabilise (warping error, 4 frame pairs)" in text
    assert "written / decoded" in text
    rows = FF.read_csv(os.path.join(d, FF.CSV_NAME))
    stab = FF.read_stabilise_csv(os.path.join(d, FF.STABILISE_CSV_NAME))
    lines = open(os.path.join(d, FF.STABILISE_CSV_NAME)).read().splitlines()
    assert len(lines) == 5 and lines[0] == "0,," and stab[0] == (None, None)
    syn = video_transfer.LAST_RUN["synthetic"]
    names = sorted(f for f in os.listdir(d) if f.endswith(".png"))
    written = [np.asarray(Image.open(os.path.join(d, f))).copy() for f in names]
    decoded = [np.asarray(Image.open(os.path.join(d0, f))).copy() for f in names]
    assert len(written) == 5
    frames, flows = syn["frames"].cpu().numpy(), syn["flows"].cpu().numpy()
    want = S.run_sequence(list(frames), decoded, [None] + [flows[t] for t in range(1, 5)])
    for t in range(5):
        assert np.array_equal(written[t], want[t]), t
    for t in range(1, 5):
        assert stab[t][1] == rows[t][0] == video_transfer.LAST_RUN["temporal"][t][0]        # one loss_out in both files
        assert stab[t][1] == mean3(temporal_loss(dev(written[t - 1]), dev(written[t]), syn["flows"][t]).cpu().numpy())
        assert stab[t][0] == plain_rows[t][0] == video_transfer.LAST_RUN["stabilised"][t][0]  # loss_raw: the run without the flag
        assert rows[t][1] == plain_rows[t][1]
        assert lines[t] == "%d,%r,%r" % (t, stab[t][0], stab[t][1])
