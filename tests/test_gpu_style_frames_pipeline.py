"""Per-frame style maps through FramePipeline and video_transfer.py ("Style maps per frame"): the ring of
style planes against the static-map route run one frame at a time, against the static FramePipeline(style_map=) run, against the
single-style runs at the end points, with planes resized on the card, together with the matte ring, and a frame whose planes
leave a pixel uncovered; then the script's --style_map_dir / --style_maps_dirs.  Frames are compared byte for byte."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import style_frames_ref as ref
from tests import test_gpu_parity as parity
from vstnet_amd.synth import synthetic_frames

pytestmark = pytest.mark.gpu
T = torch.from_numpy
H, W, N = 48, 64, 6


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """a HIP error is sticky: nothing more is started on the card once a call has failed"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                            # noqa: BLE001
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def code_shape(sp, h=H, w=W):
    return (1, 32, h, w) if sp == 2 else (1, 128, h // 2, w // 2)


def host_weights(planes, sp):
    """the shipped host route on planes at the stylised size: PIL BOX for artistic codes, then utils.style_map_weights"""
    from utils.utils import style_map_weights
    imgs = [Image.fromarray(p) for p in planes]
    if sp == 1:
        imgs = [im.resize((im.size[0] // 2, im.size[1] // 2), Image.BOX) for im in imgs]
    return style_map_weights([np.asarray(im, dtype=np.uint8) for im in imgs])


def edge_planes(P, i, h=H, w=W):
    """a vertical edge between two plateaus that moves 8 pixels per frame; P = 3 adds a constant third plane"""
    x = np.arange(w)[None, :].repeat(h, 0)
    right = x >= 8 + 8 * i
    if P == 1:
        return np.where(right, 220, 40).astype(np.uint8)[None]
    return np.stack([np.where(right, 30, 200), np.where(right, 180, 20), np.full((h, w), 60)]).astype(np.uint8)


@pytest.fixture(scope="module")
def clip():
    """per mode: net, cWCT, the statistics of three styles, sp; the frames"""
    from models.cWCT import cWCT
    frames = [(synthetic_frames(1, H, W, seed=100 + i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(N)]
    styles = [(synthetic_frames(1, 40, 56, seed=7 + k)[0].permute(1, 2, 0) * 255).byte()[None].cuda() for k in range(3)]
    out = {"frames": frames}
    for mode in ("photo", "art"):
        net, sd, sp = parity.make_net(mode)
        cw = cWCT()
        with torch.no_grad():
            stats = [cw.style_stats(net.forward_u8(s)) for s in styles]
        out[mode] = (net, cw, stats, sp)
    return out


def one_at_a_time(net, cw, stats, sp, frames, planes, mattes=None):
    """bind_style_map(host weights) -> transfer_with_stats(style_map=) -> inverse_u8, frame by frame"""
    out, routes = [], set()
    with torch.no_grad():
        for j, (f, p) in enumerate(zip(frames, planes)):
            bound = cw.bind_style_map(host_weights(p, sp), code_shape(sp), "cuda")
            kw = {}
            if mattes is not None:
                m = Image.fromarray(mattes[j])
                if sp == 1:
                    m = m.resize((W // 2, H // 2), Image.BOX)
                kw["strength"] = cw.bind_strength(np.asarray(m, dtype=np.float32) / np.float32(255), code_shape(sp), "cuda")
            z = cw.transfer_with_stats(net.forward_u8(T(f)[None].cuda()), stats, 0.0, style_map=bound, **kw)
            routes.add(cw.last_style_map)
            out.append(net.inverse_u8(z)[0].cpu().numpy())
    return out, routes


def run_pipe(net, cw, stats, frames, sink=None, **kw):
    from vstnet_amd.pipeline import FramePipeline
    run_kw = {k: kw.pop(k) for k in ("style_maps", "mattes") if k in kw}
    got, seen, routes = {}, [], set()

    def transform(z, i, strength=None, style_map=None):
        seen.append(style_map)
        if style_map is None:
            return cw.transfer_with_stats(z, stats[0], strength=strength)
        t = cw.transfer_with_stats(z, stats, 0.0, strength=strength, style_map=style_map)
        routes.add(cw.last_style_map)
        return t
    pipe = FramePipeline(net, transform, H, W, depth=2, compute_streams=2, **kw)
    n = pipe.run(iter(frames), sink or (lambda i, f: got.__setitem__(i, f.copy())), **run_kw)
    assert n == len(frames)
    return [got[i] for i in range(len(got))], pipe, seen, routes


# ------------------------------------------------------------------------------------------------ 1. the ring
@pytest.mark.parametrize("mode", ["photo", "art"])
@pytest.mark.parametrize("P", [1, 3])
def test_moving_edge_equals_one_frame_at_a_time(clip, mode, P):
    """six frames at depth 2 on two streams: every slot is reused twice"""
    net, cw, stats, sp = clip[mode]
    K = max(P, 2)
    planes = [edge_planes(P, i) for i in range(N)]
    want, want_routes = one_at_a_time(net, cw, stats[:K], sp, clip["frames"], planes)
    got, pipe, seen, routes = run_pipe(net, cw, stats[:K], clip["frames"], style_planes=P, style_maps=planes)
    assert len({id(s) for s in seen}) == 2 and all(s is not None and s.K == K for s in seen)      # one StyleMap per ring slot
    expect = "dense" if mode == "art" and K == 3 else "packed_rows"     # (artistic codes mix more than two styles densely)
    assert routes == want_routes == {expect}
    for i in range(N):
        assert np.array_equal(got[i], want[i]), i
    assert len({g.tobytes() for g in got}) == N
    with pytest.raises(ValueError, match="style_maps ran out"):
        pipe.run(iter(clip["frames"]), lambda i, f: None, style_maps=planes[:1])
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="style_maps"):
        pipe.run(iter(clip["frames"]), lambda i, f: None)
    with pytest.raises(ValueError, match="style planes must be uint8"):
        pipe.run(iter(clip["frames"]), lambda i, f: None, style_maps=[planes[0][:, :-4]] * N)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["photo", "art"])
def test_same_planes_equal_the_static_run(clip, mode):
    net, cw, stats, sp = clip[mode]
    frames = clip["frames"][:4]
    planes = edge_planes(1, 2)
    bound = cw.bind_style_map(host_weights(planes, sp), code_shape(sp), "cuda")
    static, _, seen, _ = run_pipe(net, cw, stats[:2], frames, style_map=bound)
    assert all(s is bound for s in seen)
    got, _, _, _ = run_pipe(net, cw, stats[:2], frames, style_planes=1, style_maps=[planes] * 4)
    for i in range(4):
        assert np.array_equal(got[i], static[i]), i


@pytest.mark.parametrize("mode", ["photo", "art"])
def test_end_points(clip, mode):
    """an all-0 plane is the first style alone, an all-255 plane the second: the single-style runs, byte for byte"""
    net, cw, stats, sp = clip[mode]
    frames = clip["frames"][:3]
    with torch.no_grad():
        single = [[net.inverse_u8(cw.transfer_with_stats(net.forward_u8(T(f)[None].cuda()), stats[k]))[0].cpu().numpy() for f in frames]
                  for k in range(2)]
    for k, v in ((0, 0), (1, 255)):
        got, _, _, _ = run_pipe(net, cw, stats[:2], frames, style_planes=1, style_maps=[np.full((1, H, W), v, np.uint8)] * 3)
        for i in range(3):
            assert np.array_equal(got[i], single[k][i]), (k, i)
    assert not np.array_equal(single[0][0], single[1][0])


def test_planes_resized_on_the_card(clip):
    net, cw, stats, sp = clip["photo"]
    frames = clip["frames"][:4]
    small = [np.stack([ref.planes_of(1, 30, 44, 50 + 3 * i + k, lo=1)[0] for k in range(3)]) for i in range(4)]
    big = [np.stack([ref.pil_resize_grey(p, (W, H)) for p in s]) for s in small]
    assert np.array_equal(big[0][1], np.asarray(Image.fromarray(small[0][1]).resize((W, H), Image.BILINEAR)))
    want, _, _, _ = run_pipe(net, cw, stats, frames, style_planes=3, style_maps=big)
    got, pipe, _, _ = run_pipe(net, cw, stats, frames, style_planes=3, style_hw=(30, 44), style_maps=small)
    assert pipe.d_splanes_rs is not None
    for i in range(4):
        assert np.array_equal(got[i], want[i]), i


@pytest.mark.parametrize("mode", ["photo", "art"])
def test_together_with_mattes(clip, mode):
    net, cw, stats, sp = clip[mode]
    frames = clip["frames"][:4]
    planes = [edge_planes(1, i) for i in range(4)]
    mattes = [ref.planes_of(1, H, W, 300 + i)[0] for i in range(4)]
    want, _ = one_at_a_time(net, cw, stats[:2], sp, frames, planes, mattes=mattes)
    plain, _ = one_at_a_time(net, cw, stats[:2], sp, frames, planes)
    got, pipe, _, _ = run_pipe(net, cw, stats[:2], frames, style_planes=1, style_maps=planes, mattes=mattes)
    assert pipe.strength_maps is not None and pipe.style_maps is not None            # both rings are live
    for i in range(4):
        assert np.array_equal(got[i], want[i]), i
    assert not np.array_equal(want[0], plain[0])


def test_a_zero_sum_frame_raises_when_it_retires(clip):
    from vstnet_amd.pipeline import StyleMapZeroSum
    net, cw, stats, sp = clip["photo"]
    planes = [edge_planes(3, i) for i in range(N)]
    planes[3] = planes[3].copy()
    planes[3][:, 17, 33] = 0
    reached = []
    with pytest.raises(ValueError, match="frame 3") as e:
        run_pipe(net, cw, stats, clip["frames"], sink=lambda i, f: reached.append(i), style_planes=3, style_maps=planes)
    torch.cuda.synchronize()                 # (the frame the aborted run had queued behind it)
    assert isinstance(e.value, StyleMapZeroSum) and e.value.index == 3 and "every plane" in str(e.value)
    assert reached == [0, 1, 2]


def test_constructor_exclusions(clip):
    from vstnet_amd.pipeline import FramePipeline
    net, cw, stats, sp = clip["photo"]
    tf = lambda z, i, **kw: z      # noqa: E731
    bound = cw.bind_style_map(host_weights(edge_planes(1, 0), sp), code_shape(sp), "cuda")
    for kw in (dict(style_map=bound), dict(segmenter=object()), dict(stats_by_label=True, stats_window=2), dict(style_planes=9),
               dict(style_planes=0), dict(style_hw=(2000, 64))):           # (a shrink past the device resize's 16x)
        with pytest.raises(ValueError):
            FramePipeline(net, tf, H, W, **{"style_planes": 2, **kw})
    with pytest.raises(ValueError):
        FramePipeline(net, tf, H, W, style_hw=(30, 44))                              # style_hw without style_planes
    pipe = FramePipeline(net, tf, H, W, style_planes=2)
    with pytest.raises(ValueError, match="masked routes"):
        pipe.run(iter([]), lambda i, f: None, style_maps=[], masks=[])


# ------------------------------------------------------------------------------------------------ 2. the script
def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


def _script_clip(tmp_path, n=4, h=60, w=80):
    fd = tmp_path / "clip"
    fd.mkdir()
    for i in range(n):
        parity._png(fd / f"{i:03d}.png", h, w, 40 + i)
    for k in range(3):
        parity._png(tmp_path / f"s{k}.png", 40 - 4 * k, 56, 6 + k)
    base = ["--video", str(fd), "--synthetic_weights", "--frames_only", "--max_size", "48"]
    return base, ["--styles"] + [str(tmp_path / f"s{k}.png") for k in range(3)]


@pytest.mark.parametrize("resize", ["host", "device"])
def test_script_style_map_dir_equals_style_map(tmp_path, resize):
    """one identical map per frame = --style_map with that file, PNG bytes; frames and maps 80 x 60, stylised at 48 x 36"""
    import video_transfer
    base, styles = _script_clip(tmp_path)
    md = tmp_path / "maps"
    md.mkdir()
    plane = ref.planes_of(1, 60, 80, 1)[0]
    Image.fromarray(plane).save(tmp_path / "m.png")
    for i in range(4):
        Image.fromarray(plane).save(md / f"{i:03d}.png")
    run = lambda out, *extra: _files(video_transfer.main(base + styles[:3] + ["--resize", resize, "--out_dir", str(tmp_path / out)]     # noqa: E731
                                                         + list(extra)))
    per_frame = run("dir", "--style_map_dir", str(md))
    static = run("map", "--style_map", str(tmp_path / "m.png"))
    assert sorted(per_frame) == ["%05d.png" % i for i in range(4)]
    assert per_frame == static and len(set(per_frame.values())) == 4


def test_script_with_the_flags_the_static_map_works_with(tmp_path):
    """--alpha_c, --strength_map, --preserve_luminance and --stats_window on top: still the static map's bytes"""
    import video_transfer
    base, styles = _script_clip(tmp_path)
    md = tmp_path / "maps"
    md.mkdir()
    plane = ref.planes_of(1, 60, 80, 2)[0]
    Image.fromarray(plane).save(tmp_path / "m.png")
    Image.fromarray(ref.planes_of(1, 60, 80, 3)[0]).save(tmp_path / "s.png")
    for i in range(4):
        Image.fromarray(plane).save(md / f"{i:03d}.png")
    more = ["--alpha_c", "0.3", "--strength_map", str(tmp_path / "s.png"), "--preserve_luminance", "--stats_window", "2"]
    run = lambda out, *extra: _files(video_transfer.main(base + styles[:3] + more + ["--out_dir", str(tmp_path / out)] + list(extra)))     # noqa: E731
    per_frame = run("dir", "--style_map_dir", str(md))
    assert per_frame == run("map", "--style_map", str(tmp_path / "m.png")) and len(set(per_frame.values())) == 4


def test_script_shards_read_their_own_planes(tmp_path):
    import video_transfer
    from vstnet_amd.sharding import shard_range
    base, styles = _script_clip(tmp_path)
    md = tmp_path / "maps"
    md.mkdir()
    for i in range(4):
        Image.fromarray(ref.planes_of(1, 60, 80, 70 + i)[0]).save(md / f"{i:03d}.png")
    args = base + styles[:3] + ["--style_map_dir", str(md)]
    one = _files(video_transfer.main(args + ["--out_dir", str(tmp_path / "one")]))
    assert sorted(video_transfer.LAST_RUN["style_maps"]) == list(range(4))
    for r in range(2):
        two_dir = video_transfer.main(args + ["--out_dir", str(tmp_path / "two"), "--shard", f"{r}/2"])
    assert sorted(video_transfer.LAST_RUN["style_maps"]) == list(range(*shard_range(4, 1, 2)))
    assert _files(two_dir) == one and len(set(one.values())) == 4


def test_script_three_directories_and_a_zero_sum_frame(tmp_path, capsys):
    """--style_maps_dirs with three styles: frame 0 is the library composition; then frame 2 loses a pixel and the run ends
    with a message that names the frame and its files.  Frames of 48 x 36: written at the size they are stylised at (a frame
    that --max_size shrinks is written at the reference's writer size, another one)"""
    import image_transfer
    import video_transfer
    from models.cWCT import cWCT
    from utils.utils import img_resize, to_tensor_u8
    base, styles = _script_clip(tmp_path, h=36, w=48)
    dirs = [tmp_path / f"w{k}" for k in range(3)]
    for k, d in enumerate(dirs):
        d.mkdir()
        for i in range(4):
            Image.fromarray(ref.planes_of(1, 36, 48, 10 * k + i, lo=1)[0]).save(d / f"{i:03d}.png")
    args = base + styles + ["--style_maps_dirs"] + [str(d) for d in dirs]
    out = video_transfer.main(args + ["--out_dir", str(tmp_path / "o")])
    assert sorted(_files(out)) == ["%05d.png" % i for i in range(4)]
    net = image_transfer.build_network("photorealistic", None, True, torch.device("cuda"))
    cw = cWCT()
    with torch.no_grad():
        stats = [cw.style_stats(net.forward_u8(to_tensor_u8(img_resize(Image.open(tmp_path / f"s{k}.png").convert("RGB"), 48, 4)).cuda()))
                 for k in range(3)]
        frame = img_resize(Image.open(tmp_path / "clip" / "000.png").convert("RGB"), 48, 4)
        assert frame.size == (48, 36)
        weights = image_transfer.load_style_map([str(d / "000.png") for d in dirs], (48, 36), "photorealistic")
        bound = cw.bind_style_map(weights, (1, 32, 36, 48), "cuda")
        want = net.inverse_u8(cw.transfer_with_stats(net.forward_u8(to_tensor_u8(frame).cuda()), stats, 0.0, style_map=bound))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "00000.png"))), want[0].cpu().numpy())
    for d in dirs:
        p = np.asarray(Image.open(d / "002.png")).copy()
        p[5, 9] = 0
        Image.fromarray(p).save(d / "002.png")
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        video_transfer.main(args + ["--out_dir", str(tmp_path / "z")])
    msg = str(e.value.code)
    assert "frame 2" in msg and "every plane" in msg and all(str(d / "002.png") in msg for d in dirs)
