"""FramePipeline(affinity=True), video_transfer.py --affinity and image_transfer.py --affinity on the card: the written bytes do not
change, every frame's values are those of vstnet_amd.matting.matting_loss called by hand on the same content and stylised frame
(bit for bit: the same kernel on the same inputs, whatever ring slot and stream the frame had), the guided route reports both
sizes, and the shards' files join into the file one process writes."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from test_gpu_guided_pipeline import DEPTH, H, HS, MAX_SIZE, W, WS, frames, make_pipe, setup  # noqa: F401  (setup: the fixture)

pytestmark = pytest.mark.gpu

N = 5


def work_frames(n, seed=0):
    """n frames at the working size (64 x 96 would do as well: the smallest the pipeline takes is 8 x 8)"""
    return [np.ascontiguousarray(f[:H, :W]) for f in frames(n, seed)]


def test_plain_route_same_bytes_and_values_by_hand(setup):
    from vstnet_amd.matting import matting_loss
    from vstnet_amd.pipeline import FramePipeline
    net, tf = setup
    src = work_frames(N)
    plain, got = [], []
    FramePipeline(net, tf, H, W, depth=DEPTH).run(src, lambda i, a: plain.append(a.copy()))
    pipe = FramePipeline(net, tf, H, W, depth=DEPTH, affinity=True)
    assert pipe.run(src, lambda i, a: got.append(a.copy())) == N
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    assert sorted(pipe.affinity) == list(range(N))
    for i in range(N):
        v = pipe.affinity[i]
        assert v.shape == (3,) and v.dtype == np.float64 and np.isfinite(v).all() and (v > 0).all()
        want = matting_loss(torch.from_numpy(src[i]).cuda(), torch.from_numpy(got[i]).cuda()).cpu().numpy()
        assert v.tobytes() == want.tobytes(), (i, v, want)
    assert len({pipe.affinity[i].tobytes() for i in range(N)}) == N         # (frames that all differ: a stale slot cannot hide)
    # the radius and the ridge reach the kernel; the Lab step's route measures its own written frame
    p2 = FramePipeline(net, tf, H, W, depth=DEPTH, affinity=True, affinity_radius=2, affinity_eps=1e-5, preserve_luminance=True)
    got2 = []
    p2.run(src[:2], lambda i, a: got2.append(a.copy()))
    for i in range(2):
        want = matting_loss(torch.from_numpy(src[i]).cuda(), torch.from_numpy(got2[i]).cuda(), 2, 1e-5).cpu().numpy()
        assert p2.affinity[i].tobytes() == want.tobytes()
    # without the keyword nothing is made
    off = FramePipeline(net, tf, H, W, depth=DEPTH)
    assert off.aff_work is None and off.d_affinity is None and off.affinity == {}


def test_guided_route_reports_both_sizes(setup):
    from vstnet_amd.color import luminance_transfer_u8  # noqa: F401
    from vstnet_amd.matting import matting_loss
    from vstnet_amd.resize import DeviceImgResize
    net, tf = setup
    src = frames(N)
    plain, got = [], []
    make_pipe(net, tf).run(src, lambda i, a: plain.append(a.copy()))
    pipe = make_pipe(net, tf, affinity=True)
    pipe.run(src, lambda i, a: got.append(a.copy()))
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    dev = torch.device("cuda")
    for i in range(N):
        v = pipe.affinity[i]
        assert v.shape == (6,) and np.isfinite(v).all()
        with torch.no_grad():
            s = torch.from_numpy(src[i]).cuda()
            d_in = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
            DeviceImgResize((HS, WS), MAX_SIZE, 4, dev)(s, d_in)
            sty = net(tf(net.forward_u8(d_in), i), forward=False)
            work = matting_loss(d_in, sty).cpu().numpy()
            full = matting_loss(s, torch.from_numpy(got[i]).cuda()).cpu().numpy()
        assert v[:3].tobytes() == work.tobytes() and v[3:].tobytes() == full.tobytes(), (i, v, work, full)


def test_constructor_errors(setup):
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.yuv import DeepYuvSpec
    net, tf = setup
    with pytest.raises(ValueError, match="high-bit-depth out_yuv"):
        FramePipeline(net, tf, H, W, affinity=True, out_yuv=DeepYuvSpec("420mpeg2", "bt709", "limited", 10))
    with pytest.raises(ValueError, match="out_height, out_width"):
        FramePipeline(net, tf, H, W, affinity=True, out_height=HS, out_width=WS, decode=lambda z: None)
    with pytest.raises(ValueError, match="radius"):
        FramePipeline(net, tf, H, W, affinity=True, affinity_radius=4)
    with pytest.raises(ValueError, match="eps"):
        FramePipeline(net, tf, H, W, affinity=True, affinity_eps=0.0)


def test_video_script_csv_and_shards(tmp_path, capsys):
    import video_transfer
    from vstnet_amd import affinity as A
    fd = tmp_path / "clip"
    fd.mkdir()
    for i, f in enumerate(frames(N, seed=2)):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
    Image.fromarray(frames(1, seed=3)[0][:48, :64].copy()).save(tmp_path / "s.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--max_size", str(MAX_SIZE), "--synthetic_weights",
            "--frames_only", "--resize", "device", "--upscale", "guided"]

    def run(name, extra):
        d = video_transfer.main(base + ["--out_dir", str(tmp_path / name)] + extra)
        return d, [np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d)) if f.endswith(".png")]
    d_plain, plain = run("plain", [])
    assert not os.path.exists(os.path.join(d_plain, A.CSV_NAME)) and "affinity" not in video_transfer.LAST_RUN
    capsys.readouterr()
    d_one, one = run("one", ["--affinity"])
    text = capsys.readouterr().out
    assert "affinity (Matting-Laplacian loss, 5 frames)" in text and "working size mean" in text and "full size mean" in text
    assert len(one) == N and all(np.array_equal(a, b) for a, b in zip(plain, one))
    rows = A.read_csv(os.path.join(d_one, A.CSV_NAME))
    assert sorted(rows) == list(range(N)) and all(len(v) == 2 and v[0] > 0 and v[1] > 0 for v in rows.values())
    assert video_transfer.LAST_RUN["affinity"] == rows
    lines = open(os.path.join(d_one, A.CSV_NAME)).read().splitlines()
    assert [ln.split(",")[0] for ln in lines] == [str(i) for i in range(N)]
    d0, _ = run("sh", ["--affinity", "--shard", "0/2"])
    d1, _ = run("sh", ["--affinity", "--shard", "1/2"])
    assert d0 == d1 and not os.path.exists(os.path.join(d0, A.CSV_NAME))
    joined = A.join_parts([os.path.join(d0, A.part_name(1)), os.path.join(d0, A.part_name(0))], tmp_path / "joined.csv", N)
    assert open(joined, "rb").read() == open(os.path.join(d_one, A.CSV_NAME), "rb").read()
    # the working size alone, on the route that decodes straight to uint8
    d_w, _ = run("work", ["--affinity", "--upscale", "bicubic", "--max_size", "1280"])
    assert all(len(v) == 1 for v in A.read_csv(os.path.join(d_w, A.CSV_NAME)).values())


def test_video_parser_errors(tmp_path):
    import video_transfer
    Image.fromarray(frames(1)[0]).save(tmp_path / "000.png")
    base = ["--video", str(tmp_path), "--style", str(tmp_path / "000.png"), "--out_dir", str(tmp_path / "o"), "--affinity"]
    for extra in (["--affinity_radius", "4"], ["--affinity_eps", "0"], ["--stub_stylise"]):
        with pytest.raises(SystemExit) as e:
            video_transfer.main(base + extra)
        assert e.value.code == 2


def test_image_script_prints_and_writes_the_map(tmp_path, capsys):
    import image_transfer
    src, style = frames(1, seed=4)[0], frames(1, seed=5)[0][:48, :64].copy()
    Image.fromarray(src).save(tmp_path / "c.png")
    Image.fromarray(style).save(tmp_path / "s.png")
    base = ["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--max_size", str(MAX_SIZE),
            "--synthetic_weights"]
    plain = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "p")])))
    capsys.readouterr()
    got = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "a"), "--affinity", "--affinity_map",
                                                            str(tmp_path / "heat.png")])))
    text = capsys.readouterr().out
    assert np.array_equal(plain, got) and "affinity (Matting-Laplacian loss" in text
    value = image_transfer.LAST_RUN["affinity"]["work"]
    assert value > 0 and ("%.6e" % value) in text
    heat = Image.open(tmp_path / "heat.png")
    assert heat.mode == "L" and heat.size == (W, H) and np.asarray(heat).max() == 255
    # both sizes under --upscale guided; the map keeps the stylised size
    image_transfer.main(base + ["--out_dir", str(tmp_path / "g"), "--upscale", "guided", "--affinity", "--affinity_map",
                                str(tmp_path / "heat2.png")])
    text = capsys.readouterr().out
    m = image_transfer.LAST_RUN["affinity"]
    assert m["work"] > 0 and m["full"] > 0 and "full size %dx%d" % (WS, HS) in text
    assert Image.open(tmp_path / "heat2.png").size == (W, H)
    with pytest.raises(SystemExit):
        image_transfer.main(base + ["--out_dir", str(tmp_path / "x"), "--affinity_map", str(tmp_path / "h.png")])
