"""Per-frame strength maps on the GPU: vst_strength_frame against its numpy restatement, bit for bit;
vst_resize_grey_u8 against Pillow, byte for byte; FramePipeline's matte / label rings against the static-map route run one frame
at a time, byte for byte; the scripts' --strength_dir / --strength_labels against --strength_map and the library.  No tolerance
anywhere: every comparison is equality."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import strength_frames_ref as ref
from tests import test_gpu_parity as parity
from tests.zc import ptr, stream
from vstnet_amd import _lib
from vstnet_amd.synth import SEG_DEPTHS, synthetic_frames, synthetic_scene_u8, synthetic_segformer_state_dict

pytestmark = pytest.mark.gpu
T = torch.from_numpy
make_net = parity.make_net
RESIZES = [((23, 37), (12, 16)), ((12, 16), (28, 40)), ((23, 37), (23, 16)), ((256, 256), (16, 16))]


def table_of(seed=0):
    """256 distinct strengths in [0, 1], 0 and 1 among them"""
    t = np.random.default_rng(seed).permutation(256).astype(np.float32) / np.float32(255)
    assert t.min() == 0.0 and t.max() == 1.0 and len(np.unique(t)) == 256
    return t


def matte_of(H, W, seed):
    """a matte that cycles through a permutation of the 256 byte values (all of them where the frame has 256 pixels)"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.permutation(256) for _ in range((H * W + 255) // 256)])[:H * W]
    return rng.permutation(v).astype(np.uint8).reshape(H, W)


def run_kernel(matte, labels, table, H, W, sp, dense=True, rows=True):
    n = H * W if sp == 2 else H * W // 4
    dm = None if matte is None else T(matte).cuda()
    dl = None if labels is None else T(labels).cuda()
    dt = None if labels is None else T(table).cuda()
    # (poisoned outputs: every element must be written)
    dd = torch.full((n,), -7.0, device="cuda") if dense else None
    dr = torch.full((n,), -7.0, device="cuda") if rows else None
    p = lambda t: ptr(t) if t is not None else None        # noqa: E731
    _lib.check(_lib.lib().vst_strength_frame(p(dm), p(dl), p(dt), p(dd), p(dr), H, W, sp, stream()), "vst_strength_frame")
    return (None if dd is None else dd.cpu().numpy()), (None if dr is None else dr.cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. kernel, bit for bit
@pytest.mark.parametrize("sp", [2, 1])
@pytest.mark.parametrize("H,W", [(8, 8), (12, 20), (64, 48)])
@pytest.mark.parametrize("inputs", ["matte", "labels", "both"])
def test_kernel_equals_the_restatement(sp, H, W, inputs):
    matte = matte_of(H, W, H + sp) if inputs != "labels" else None
    labels = np.random.default_rng(W).integers(0, 256, (H, W), dtype=np.uint8) if inputs != "matte" else None
    table = table_of(3)
    if matte is not None and H * W >= 256:
        assert len(np.unique(matte)) == 256
    want = ref.strength_frame(matte, labels, table, sp)
    assert want.dtype == np.float32 and want.shape == ((H, W) if sp == 2 else (H // 2, W // 2))
    dense, rows = run_kernel(matte, labels, table, H, W, sp)
    assert np.array_equal(bits(dense), bits(want.reshape(-1)))
    assert np.array_equal(bits(rows), bits(ref.rows_of(want, H, W, sp)))
    # rows = vst_map_to_code(dense), the library's own permutation
    d = T(dense).cuda()
    r = torch.empty_like(d)
    _lib.check(_lib.lib().vst_map_to_code(ptr(d), ptr(r), H, W, sp, stream()), "vst_map_to_code")
    assert np.array_equal(bits(r.cpu().numpy()), bits(rows))
    # either output alone
    d_only, none = run_kernel(matte, labels, table, H, W, sp, rows=False)
    assert none is None and np.array_equal(bits(d_only), bits(dense))
    none, r_only = run_kernel(matte, labels, table, H, W, sp, dense=False)
    assert none is None and np.array_equal(bits(r_only), bits(rows))


@pytest.mark.parametrize("sp", [2, 1])
def test_all_256_matte_values(sp):
    """v / 255 for every byte: the float of np.float32(v) / np.float32(255); for artistic codes through constant 2 x 2 blocks"""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    matte = v if sp == 2 else np.repeat(np.repeat(v, 2, 0), 2, 1)
    H, W = matte.shape
    dense, _ = run_kernel(matte, None, None, H, W, sp)
    assert np.array_equal(bits(dense), bits(np.arange(256, dtype=np.float32) / np.float32(255)))
    assert dense[0] == 0.0 and dense[255] == 1.0


# ------------------------------------------------------------------------------------------------ 2. grey resize = Pillow
@pytest.mark.parametrize("src,dst", RESIZES)
def test_resize_grey_is_pillows(src, dst):
    from vstnet_amd import resize
    img = ref.grey(src[0], src[1], 5)
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
    got = resize.resize_grey_u8(T(img).cuda(), (dst[1], dst[0]))
    assert tuple(got.shape) == dst and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ref.pil_resize_grey(img, (dst[1], dst[0])), want)
    same = resize.resize_grey_u8(T(img).cuda(), (src[1], src[0]))
    assert np.array_equal(same.cpu().numpy(), img)
    with pytest.raises(ValueError):
        resize.resize_grey_u8(T(img), (dst[1], dst[0]))
    with pytest.raises(ValueError):
        resize.resize_grey_u8(T(img).cuda().float(), (dst[1], dst[0]))


# ------------------------------------------------------------------------------------------------ 3 / 4. the matte ring
H3, W3, N3 = 32, 48, 7


@pytest.fixture(scope="module")
def clip3():
    """per mode: net, cWCT, style statistics, the frames and, once, the frames of a run without any strength"""
    from models.cWCT import cWCT
    frames = [(synthetic_frames(1, H3, W3, seed=100 + i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(N3)]
    style = (synthetic_frames(1, 40, 56, seed=7)[0].permute(1, 2, 0) * 255).byte()[None].cuda()
    out = {"frames": frames}
    for mode in ("photo", "art"):
        net, sd, sp = make_net(mode)
        cw = cWCT()
        with torch.no_grad():
            stats = cw.style_stats(net.forward_u8(style))
            plain = [net.inverse_u8(cw.transfer_with_stats(net.forward_u8(T(f)[None].cuda()), stats))[0].cpu().numpy() for f in frames]
        out[mode] = (net, cw, stats, sp, plain)
    return out


def code_shape(sp, H, W):
    return (1, 32, H, W) if sp == 2 else (1, 128, H // 2, W // 2)


def host_map(matte, H, W, sp):
    """what load_strength_map makes of the same image, with Pillow itself"""
    img = Image.fromarray(matte)
    if img.size != (W, H):
        img = img.resize((W, H), Image.BILINEAR)
    if sp == 1:
        img = img.resize((W // 2, H // 2), Image.BOX)
    return np.asarray(img, dtype=np.float32) / np.float32(255)


def one_at_a_time(net, cw, stats, sp, frames, maps):
    """bind_strength -> transfer_with_stats(strength=) -> inverse_u8, frame by frame"""
    out = []
    with torch.no_grad():
        for f, m in zip(frames, maps):
            sm = cw.bind_strength(m, code_shape(sp, f.shape[0], f.shape[1]), "cuda")
            out.append(net.inverse_u8(cw.transfer_with_stats(net.forward_u8(T(f)[None].cuda()), stats, strength=sm))[0].cpu().numpy())
    return out


def run_pipe(net, transform, frames, H, W, **kw):
    from vstnet_amd.pipeline import FramePipeline
    run_kw = {k: kw.pop(k) for k in ("masks", "mattes") if k in kw}
    got = {}
    pipe = FramePipeline(net, transform, H, W, depth=3, compute_streams=2, **kw)
    assert pipe.run(iter(frames), lambda i, f: got.__setitem__(i, f.copy()), **run_kw) == len(frames)
    return [got[i] for i in range(len(frames))], pipe


@pytest.mark.parametrize("mode", ["photo", "art"])
@pytest.mark.parametrize("matte_hw", [(H3, W3), (50, 70)])
def test_matte_ring_equals_one_frame_at_a_time(clip3, mode, matte_hw):
    net, cw, stats, sp, plain = clip3[mode]
    frames = clip3["frames"]
    mattes = [ref.grey(matte_hw[0], matte_hw[1], 200 + i) for i in range(N3)]
    want = one_at_a_time(net, cw, stats, sp, frames, [host_map(m, H3, W3, sp) for m in mattes])
    calls = []

    def transform(z, i, strength=None):
        calls.append(strength)
        return cw.transfer_with_stats(z, stats, strength=strength)
    got, pipe = run_pipe(net, transform, frames, H3, W3, mattes=mattes, matte_hw=matte_hw)
    assert len({id(s) for s in calls}) == 3 and all(s is not None for s in calls)          # one StrengthMap per ring slot
    for i in range(N3):
        assert np.array_equal(got[i], want[i]), i
    assert any(not np.array_equal(got[i], plain[i]) for i in range(N3))
    with pytest.raises(ValueError, match="mattes ran out"):
        pipe.run(iter(frames), lambda i, f: None, mattes=mattes[:2])
    torch.cuda.synchronize()                 # (the two frames the aborted run had queued)
    # a run without mattes afterwards: the plain calls again
    n_calls = len(calls)
    got2 = {}
    pipe.run(iter(frames[:2]), lambda i, f: got2.__setitem__(i, f.copy()))
    assert calls[n_calls:] == [None, None] and np.array_equal(got2[0], plain[0])


@pytest.mark.parametrize("mode", ["photo", "art"])
def test_end_points(clip3, mode):
    net, cw, stats, sp, plain = clip3[mode]
    frames = clip3["frames"][:4]
    tf = lambda z, i, strength=None: cw.transfer_with_stats(z, stats, strength=strength)      # noqa: E731
    white, _ = run_pipe(net, tf, frames, H3, W3, mattes=[np.full((H3, W3), 255, np.uint8)] * 4)
    black, _ = run_pipe(net, tf, frames, H3, W3, mattes=[np.zeros((H3, W3), np.uint8)] * 4)
    cH, cW = code_shape(sp, H3, W3)[2:]
    zeros = one_at_a_time(net, cw, stats, sp, frames, [np.zeros((cH, cW), np.float32)] * 4)
    for i in range(4):
        assert np.array_equal(white[i], plain[i]), i
        assert np.array_equal(black[i], zeros[i]), i


# ------------------------------------------------------------------------------------------------ 5. labels
def bands(h, w, labels, shift=0):
    edges = np.linspace(0, w, len(labels) + 1).astype(int)
    m = np.zeros((h, w), np.uint8)
    for k, l in enumerate(labels):
        m[:, edges[k]: edges[k + 1]] = l
    return np.ascontiguousarray(np.roll(m, shift, axis=1))


@pytest.mark.parametrize("with_matte,colours", [(False, False), (True, False), (False, True)])
def test_label_strengths_equal_the_static_route(with_matte, colours):
    """per-frame maps of 3 labels, table {1: 0, 2: 0.5}; frame 2 has 9 label bands and is done again on the dense route"""
    from models.cWCT import cWCT
    from utils.utils import SEG_COLORS
    H, W, n = 64, 64, 4
    net, sd, sp = make_net("photo")
    cw = cWCT()
    frames = [(synthetic_frames(1, H, W, seed=300 + i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(n)]
    style = (synthetic_frames(1, H, W, seed=9)[0].permute(1, 2, 0) * 255).byte()[None].cuda()
    nine = list(range(9))
    maps = [bands(H, W, [0, 1, 2], 5 * i) for i in range(n)]
    maps[2] = bands(H, W, nine)
    mattes = [ref.grey(H, W, 400 + i) for i in range(n)] if with_matte else None
    table = cWCT.strength_table({1: 0.0, 2: 0.5})
    tab = table.numpy()
    colour_of = {v: c for c, v in SEG_COLORS}
    uploads = [np.array([colour_of[v] for v in range(9)], np.uint8)[m] for m in maps] if colours else maps
    with torch.no_grad():
        binding = cw.bind_style_labels(net.forward_u8(style), bands(H, W, nine)[None])
        want = []
        for i in range(n):
            z = net.forward_u8(T(frames[i])[None].cuda())
            s = tab[maps[i]]
            if with_matte:
                s = (mattes[i].astype(np.float32) / np.float32(255)) * s
            sm = cw.bind_strength(s, (1, 32, H, W), "cuda")
            cap = 32 if i == 2 else 8
            want.append(net.inverse_u8(cw.transfer_with_plan(z, None, cw.plan_frame(T(maps[i]).cuda(), binding, max_slots=cap),
                                                             strength=sm))[0].cpu().numpy())
            plain2 = net.inverse_u8(cw.transfer_with_plan(z, None, cw.plan_frame(T(maps[i]).cuda(), binding, max_slots=cap)))
        assert not np.array_equal(want[-1], plain2[0].cpu().numpy())                    # the table changes the frame

    def planned(cap):
        def transform(z, i, ms, strength=None):
            assert strength is not None
            buf = ms.state.get("buffers")
            if buf is None:
                buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, "cuda")
            return cw.transfer_with_plan(z, None, cw.plan_frame(ms.mask, binding, colours=ms.colours, max_slots=cap, buffers=buf,
                                                                flags=ms.flags), strength=strength)
        return transform
    kw = dict(mattes=mattes) if with_matte else {}
    got, pipe = run_pipe(net, planned(8), frames, H, W, redo=planned(32), strength_table=table, masks=uploads, **kw)
    assert pipe.redo_count == 1
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i


def test_strength_table_needs_a_label_source():
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    net, sd, sp = make_net("photo")
    pipe = FramePipeline(net, lambda z, i, strength=None: z, 32, 48, strength_table=cWCT.strength_table("1:0.5"))
    with pytest.raises(ValueError, match="label source"):
        pipe.run(iter([np.zeros((32, 48, 3), np.uint8)]), lambda i, f: None)
    with pytest.raises(ValueError):
        FramePipeline(net, lambda z, i: z, 32, 48, strength_table=np.ones(255, np.float32))
    with pytest.raises(ValueError):
        cWCT.frame_strength((1, 32, 32, 48), labels=torch.zeros((32, 48), dtype=torch.uint8, device="cuda"))       # no table
    with pytest.raises(ValueError):
        cWCT.frame_strength((1, 32, 32, 48), matte=torch.zeros((32, 44), dtype=torch.uint8, device="cuda"))       # wrong shape


# ------------------------------------------------------------------------------------------------ 6. segmenter
@pytest.mark.parametrize("window", [1, 2])
def test_segmenter_labels_through_the_table(window):
    from models.cWCT import cWCT
    from vstnet_amd.segformer import SegFormer
    H, W, n = 64, 64, 4
    seg = SegFormer("b1", embedding_dim=256).load_state_dict(synthetic_segformer_state_dict(4321, SEG_DEPTHS["b1"], 256))
    net, sd, sp = make_net("photo")
    cw = cWCT()
    frames = [synthetic_scene_u8(H, W, 40 + i) for i in range(n)]
    style = (synthetic_frames(1, 48, 64, seed=7)[0].permute(1, 2, 0) * 255).byte()[None].cuda()
    table = T(table_of(5))
    tab = table.numpy()
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(style))
    seen = {}
    tf = lambda z, i, ms, strength=None: cw.transfer_with_stats(z, stats, strength=strength)      # noqa: E731
    got, pipe = run_pipe(net, tf, frames, H, W, segmenter=seg, strength_table=table, seg_window=window,
                         mask_sink=lambda i, m: seen.__setitem__(i, m.copy()))
    with torch.no_grad():
        if window == 1:
            labels = [seg.segment_u8(T(f).cuda()).cpu().numpy() for f in frames]
            for i in range(n):
                assert np.array_equal(seen[i], labels[i]), i
        else:           # the windowed labels, as the sink got them (no remapping table in this run)
            labels = [seen[i] for i in range(n)]
            assert np.array_equal(labels[0], seg.segment_u8(T(frames[0]).cuda()).cpu().numpy())     # (frame 0 has no history)
        assert len(np.unique(np.concatenate([l.reshape(-1) for l in labels]))) > 1, "one label everywhere tests no lookup"
    want = one_at_a_time(net, cw, stats, sp, frames, [tab[l] for l in labels])
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i


# ------------------------------------------------------------------------------------------------ 7. scripts
def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


@pytest.mark.parametrize("resize", ["host", "device"])
def test_video_script_strength_dir_equals_strength_map(tmp_path, resize):
    """one identical map per frame = --strength_map with that file, PNG bytes; frames and maps 80 x 60, stylised at 48 x 36"""
    import video_transfer
    fd, md = tmp_path / "clip", tmp_path / "mattes"
    fd.mkdir()
    md.mkdir()
    matte = ref.grey(60, 80, 1)
    Image.fromarray(matte).save(tmp_path / "m.png")
    for i in range(4):
        parity._png(fd / f"{i:03d}.png", 60, 80, 40 + i)
        Image.fromarray(matte).save(md / f"{i:03d}.png")
    parity._png(tmp_path / "s.png", 40, 56, 6)
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only", "--max_size", "48",
            "--resize", resize]
    run = lambda out, *extra: video_transfer.main(base + ["--out_dir", str(tmp_path / out)] + list(extra))      # noqa: E731
    per_frame = _files(run("dir", "--strength_dir", str(md)))
    static = _files(run("map", "--strength_map", str(tmp_path / "m.png")))
    none = _files(run("none"))
    assert sorted(per_frame) == ["%05d.png" % i for i in range(4)]
    assert per_frame == static
    assert all(per_frame[f] != none[f] for f in per_frame)


def test_video_script_shards_read_their_own_mattes(tmp_path):
    import video_transfer
    fd, md = tmp_path / "clip", tmp_path / "mattes"
    fd.mkdir()
    md.mkdir()
    for i in range(5):
        parity._png(fd / f"{i:03d}.png", 48, 64, 40 + i)
        Image.fromarray(ref.grey(48, 64, 70 + i)).save(md / f"{i:03d}.png")
    parity._png(tmp_path / "s.png", 40, 56, 6)
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only", "--strength_dir", str(md)]
    one = _files(video_transfer.main(base + ["--out_dir", str(tmp_path / "one")]))
    assert sorted(video_transfer.LAST_RUN["mattes"]) == list(range(5))
    for r in range(2):
        two_dir = video_transfer.main(base + ["--out_dir", str(tmp_path / "two"), "--shard", f"{r}/2"])
    from vstnet_amd.sharding import shard_range
    assert sorted(video_transfer.LAST_RUN["mattes"]) == list(range(*shard_range(5, 1, 2)))
    assert _files(two_dir) == one and len(set(one.values())) == 5


def test_image_script_strength_labels(tmp_path):
    """image_transfer.py --strength_labels: the bytes of the static-map route with table[labels] built on the host; in the code
    the named label's pixels change and - the table's default being 1 - no other pixel does.  The decoded image differs
    beyond the label too, because the decoder's convolutions spread every code pixel over its neighbourhood, so "only there"
    is asserted where it can hold, in the code.  Measured on an MI355X, 48 x 64, label 1 on 1008 pixels: code pixels that
    differ 1008 of 1008 on the label and 0 of 2064 off it; decoded pixels 1008 of 1008 on it and 1445 of 2064 off it."""
    import image_transfer
    from models.cWCT import cWCT
    from utils.utils import SEG_COLORS, to_tensor_u8
    H, W = 48, 64
    c = parity._png(tmp_path / "c.png", H, W, 1)
    s = parity._png(tmp_path / "s.png", H, W, 2)
    colour_of = np.array([{v: col for col, v in SEG_COLORS}[v] for v in range(9)], np.uint8)
    cseg, sseg = bands(H, W, [0, 1, 2]), bands(H, W, [2, 0, 1])
    Image.fromarray(colour_of[cseg]).save(tmp_path / "cseg.png")
    Image.fromarray(colour_of[sseg]).save(tmp_path / "sseg.png")
    base = ["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--synthetic_weights",
            "--content_seg", str(tmp_path / "cseg.png"), "--style_seg", str(tmp_path / "sseg.png")]
    with_flag = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "a"), "--strength_labels", "1:0.25"])))
    without = np.asarray(Image.open(image_transfer.main(base + ["--out_dir", str(tmp_path / "b")])))
    net, sd, sp = make_net("photo")
    cw = cWCT()
    smap = cWCT.strength_table("1:0.25").numpy()[cseg]
    with torch.no_grad():
        z, zs = net.forward_u8(to_tensor_u8(Image.fromarray(c)).cuda()), net.forward_u8(to_tensor_u8(Image.fromarray(s)).cuda())
        t = cw.transfer(z, zs, cseg[None], sseg[None], strength=smap)
        plain = cw.transfer(z, zs, cseg[None], sseg[None])
        want = net.inverse_u8(t)[0].cpu().numpy()
        a, b = (x.materialize() if hasattr(x, "materialize") else x for x in (t, plain))
        differs = (a != b).any(1)[0].cpu().numpy()
    px = (with_flag != without).any(-1)
    print("decoded pixels that differ: %d of %d on label 1, %d of %d off it; code pixels: %d of %d on it, %d off it"
          % (px[cseg == 1].sum(), (cseg == 1).sum(), px[cseg != 1].sum(), (cseg != 1).sum(), differs[cseg == 1].sum(),
             (cseg == 1).sum(), differs[cseg != 1].sum()))
    assert np.array_equal(with_flag, want)
    assert differs[cseg == 1].any() and not differs[cseg != 1].any()
    assert (with_flag != without)[cseg == 1].any()
    # the map the script's call makes is the host's, bit for bit
    sm = cWCT.frame_strength((1, 32, H, W), labels=T(cseg).cuda(), table=cWCT.strength_table("1:0.25", device="cuda"))
    assert np.array_equal(bits(sm.dense.cpu().numpy().reshape(H, W)), bits(smap))


def _clip(tmp_path, n=4, H=48, W=64):
    fd = tmp_path / "clip"
    fd.mkdir()
    frames = [parity._png(fd / f"{i:03d}.png", H, W, 40 + i) for i in range(n)]
    style = parity._png(tmp_path / "s.png", 40, 56, 6)
    white = tmp_path / "white"
    white.mkdir()
    for i in range(n):
        Image.fromarray(np.full((H, W), 255, np.uint8)).save(white / f"{i:03d}.png")
    Image.fromarray(np.full((H, W), 255, np.uint8)).save(tmp_path / "white.png")
    return fd, frames, style, white


def test_video_script_strength_labels_per_frame_maps(tmp_path):
    """--content_seg_dir + --strength_labels: the library's frames (table[labels] built on the host, the static-map route); an
    all-white --strength_dir or --strength_map on top multiplies by exactly 1"""
    import video_transfer
    from models.cWCT import cWCT
    from utils.utils import to_tensor_u8
    H, W, n = 48, 64, 4
    fd, frames, style, white = _clip(tmp_path, n, H, W)
    md = tmp_path / "maps"
    md.mkdir()
    maps = [bands(H, W, [0, 1, 2], 6 * i) for i in range(n)]
    for i, m in enumerate(maps):
        Image.fromarray(m).save(md / f"{i:03d}.png")
    sseg = bands(40, 56, [2, 0, 1])
    Image.fromarray(sseg).save(tmp_path / "sseg.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only",
            "--content_seg_dir", str(md), "--style_seg", str(tmp_path / "sseg.png")]
    run = lambda out, *extra: video_transfer.main(base + ["--out_dir", str(tmp_path / out)] + list(extra))      # noqa: E731
    out_dir = run("a", "--strength_labels", "1:0.25")
    a = _files(out_dir)
    assert a != _files(run("b"))
    assert _files(run("c", "--strength_labels", "1:0.25", "--strength_dir", str(white))) == a
    assert _files(run("d", "--strength_labels", "1:0.25", "--strength_map", str(tmp_path / "white.png"))) == a
    net, sd, sp = make_net("photo")
    cw = cWCT()
    tab = cWCT.strength_table("1:0.25").numpy()
    with torch.no_grad():
        binding = cw.bind_style_labels(net.forward_u8(to_tensor_u8(Image.fromarray(style)).cuda()), sseg[None])
        for i in range(n):
            z = net.forward_u8(to_tensor_u8(Image.fromarray(frames[i])).cuda())
            t = cw.transfer_with_plan(z, None, cw.plan_frame(T(maps[i]).cuda(), binding, max_slots=8), strength=tab[maps[i]])
            got = np.asarray(Image.open(os.path.join(out_dir, "%05d.png" % i)))
            assert np.array_equal(got, net.inverse_u8(t)[0].cpu().numpy()), i


def test_video_script_strength_labels_one_map_for_the_clip(tmp_path):
    """--content_seg + --strength_labels {1: 0}: the frames of --strength_map with the map that is black on label 1 and white
    elsewhere; an all-white --strength_dir on top changes nothing"""
    import video_transfer
    from utils.utils import SEG_COLORS
    H, W, n = 48, 64, 4
    fd, frames, style, white = _clip(tmp_path, n, H, W)
    colour_of = np.array([{v: col for col, v in SEG_COLORS}[v] for v in range(9)], np.uint8)
    cseg, sseg = bands(H, W, [0, 1, 2]), bands(40, 56, [2, 0, 1])
    Image.fromarray(colour_of[cseg]).save(tmp_path / "cseg.png")
    Image.fromarray(colour_of[sseg]).save(tmp_path / "sseg.png")
    Image.fromarray(np.where(cseg == 1, 0, 255).astype(np.uint8)).save(tmp_path / "equiv.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only",
            "--content_seg", str(tmp_path / "cseg.png"), "--style_seg", str(tmp_path / "sseg.png")]
    run = lambda out, *extra: _files(video_transfer.main(base + ["--out_dir", str(tmp_path / out)] + list(extra)))      # noqa: E731
    a = run("a", "--strength_labels", "1:0")
    assert a == run("b", "--strength_map", str(tmp_path / "equiv.png"))
    assert a != run("c")
    assert a == run("d", "--strength_labels", "1:0", "--strength_dir", str(white))
