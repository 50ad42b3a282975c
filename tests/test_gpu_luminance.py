"""Luminance preservation at the uint8 frame edge on the card (csrc/color.hip vst_lab_luminance_u8[_f32],
RevResNet.inverse_u8(luminance_of=...), FramePipeline(preserve_luminance=True), video_transfer.py --preserve_luminance): the
kernel against the composition of the shipped float pieces bit for bit and against the oracle, the frame loop against the
one-frame-at-a-time calls bit for bit on every route, and the script end to end against the oracle."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from oracle import cpu_ref
from vstnet_amd import _lib
from vstnet_amd.synth import synthetic_state_dict, synthetic_frames

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SHAPES = [(1, 7, 13), (3, 33, 50), (2, 64, 64), (1, 1080, 1920)]


def _case(B, H, W, seed):
    """uint8 HWC content, fp32 stylised planes in [-0.3, 1.3] (both clamps of the decoder range are exercised), and the content
    as the float image a TRUE division by 255 gives (numpy on the CPU; a GPU div by a scalar may multiply by the reciprocal)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    s = torch.rand((B, 3, H, W), generator=g) * 1.6 - 0.3
    s[0, :, 0, :4] = T(np.array([[-0.3, 0.0, 1.0, 1.3]] * 3, np.float32))
    c_f = T(np.ascontiguousarray((c.numpy().astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)))
    return c, s, c_f


def _quantise(x):
    return x.mul(255).clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous()


def _offset_copy(t, elements):
    """the same values at a base that is `elements` items past an allocation's (aligned) start"""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device=t.device)
    v = buf[elements:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_kernel_is_the_composition_of_the_shipped_pieces(B, H, W):
    """luminance_px is shared by the float and the uint8-edge kernels, the content is the same float (true division), the
    quantisation is the same three operations: the bits are the same.  Not a tolerance."""
    from vstnet_amd.color import luminance_transfer, luminance_transfer_u8
    c, s, c_f = _case(B, H, W, seed=H)
    want_f = luminance_transfer(c_f.cuda(), s.cuda()).cpu()
    want_u8 = _quantise(want_f)
    cd, sd_ = c.cuda(), s.cuda()
    got_u8 = luminance_transfer_u8(cd, sd_)
    assert got_u8.dtype == torch.uint8 and tuple(got_u8.shape) == (B, H, W, 3)
    n_diff = int((got_u8.cpu() != want_u8).sum())
    print(f"u8 form {B}x{H}x{W}: {n_diff} differing bytes")
    assert n_diff == 0
    got_f = luminance_transfer_u8(cd, sd_, to_float=True)
    assert got_f.dtype == torch.float32 and tuple(got_f.shape) == (B, 3, H, W)
    assert torch.equal(got_f.cpu(), want_f)
    # bases that are not dword / 16-byte aligned take the scalar form: the same bits
    cu, su = _offset_copy(cd, 1), _offset_copy(sd_, 1)
    assert cu.data_ptr() % 4 and su.data_ptr() % 16
    assert torch.equal(luminance_transfer_u8(cu, su).cpu(), want_u8)
    assert torch.equal(luminance_transfer_u8(cu, su, to_float=True).cpu(), want_f)
    assert torch.equal(luminance_transfer_u8(cd, su).cpu(), want_u8)
    out_u = _offset_copy(torch.zeros_like(got_u8), 1)
    assert luminance_transfer_u8(cd, sd_, out=out_u) is out_u and torch.equal(out_u.cpu(), want_u8)
    # in place on the stylised planes (what the writer-size hooks do)
    s2 = sd_.clone()
    assert luminance_transfer_u8(cd, s2, out=s2, to_float=True) is s2 and torch.equal(s2.cpu(), want_f)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_kernel_against_the_oracle(B, H, W):
    """the criterion of test_image_transfer_script_preserve_luminance: every byte within one count, fewer than 2 % differ"""
    from vstnet_amd.color import luminance_transfer_u8
    c, s, c_f = _case(B, H, W, seed=H + 1)
    ref = cpu_ref.to_uint8(cpu_ref.luminance_transfer(c_f, s))
    got = luminance_transfer_u8(c.cuda(), s.cuda()).cpu()
    d = (got.int() - ref.int()).abs()
    print(f"against the oracle {B}x{H}x{W}: max diff {int(d.max())}, differing share {float((d > 0).float().mean()):.3e}")
    assert got.shape == ref.shape and int(d.max()) <= 1 and float((d > 0).float().mean()) < 2e-2


def test_argument_checks():
    from vstnet_amd.color import luminance_transfer_u8
    c, s, _ = _case(1, 8, 12, seed=3)
    with pytest.raises(RuntimeError):
        luminance_transfer_u8(c, s)                                     # no CPU path
    with pytest.raises(ValueError):
        luminance_transfer_u8(c.cuda(), s[:, :, :4].cuda())
    with pytest.raises(ValueError):
        luminance_transfer_u8(c.cuda().float(), s.cuda())
    with pytest.raises(ValueError):
        luminance_transfer_u8(c.cuda(), s.cuda(), out=torch.empty((1, 3, 8, 12), device="cuda"))      # the u8 form's out is uint8 HWC
    L = _lib.lib()
    assert L.vst_lab_luminance_u8(None, None, None, 1, 4, 4, None) == -1


# ------------------------------------------------------------------------------------------------ the decoder edge
def _net(precision=None):
    from tests.test_gpu_parity import make_net
    return make_net("photo", precision)[0]


def _frames(n, H, W, seed):
    return [(synthetic_frames(1, H, W, seed=seed + i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(n)]


def _u8(a):
    return T(np.ascontiguousarray(a))[None].cuda()


def test_inverse_u8_with_luminance_takes_every_code_form():
    """dense, PackedCode with a pending affine, PackedCode with label affines: each equals the float decode of the same code
    followed by the float blend and the quantisation; a caller's scratch holds the float decode afterwards."""
    from models.cWCT import cWCT
    from vstnet_amd.code import PackedCode
    from vstnet_amd.color import luminance_transfer
    from tests.test_gpu_masks import label_map
    net, cw = _net(), cWCT()
    H, W = 64, 96
    f = _frames(1, H, W, 300)[0]
    d = _u8(f)
    c_f = T(np.ascontiguousarray((f.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)))[None].cuda()
    seg, sty = label_map(H, W, [1, 2, 3], 3), label_map(48, 64, [1, 2, 3], 4)
    with torch.no_grad():
        z_s = net.forward_u8(_u8(_frames(1, 48, 64, 310)[0]))
        stats = cw.style_stats(z_s)
        plan = cw.bind_style(cw.learn_slots(cw.plan_masks(seg[None], sty[None], (1, 32, H, W), z_s.shape, "cuda")), z_s)
        z_c = net.forward_u8(d)
        assert isinstance(z_c, PackedCode)
        forms = {"affine": cw.transfer_with_stats(z_c, stats), "labels": cw.transfer_with_plan(net.forward_u8(d), None, plan)}
        forms["dense"] = cw.transfer_with_stats(net.forward_u8(d), stats).materialize().clone()
        assert forms["affine"].pending_affines is not None and forms["labels"].pending_labels is not None
        for name, z in forms.items():
            want_f = net(z, forward=False)
            want = _quantise(luminance_transfer(c_f, want_f))
            plain = net.inverse_u8(z)
            scratch = torch.full((1, 3, H, W), -7.0, device="cuda")
            got = net.inverse_u8(z, luminance_of=d, scratch=scratch)
            assert torch.equal(got, want), name
            assert torch.equal(scratch, want_f), name
            assert torch.equal(net.inverse_u8(z, luminance_of=d), want), name
            assert torch.equal(net.inverse_u8(z), plain) and not torch.equal(plain, got), name
        with pytest.raises(ValueError):
            net.inverse_u8(forms["dense"], luminance_of=d, scratch=torch.empty((1, 3, H, W + 4), device="cuda"))
        with pytest.raises(ValueError):
            net.inverse_u8(forms["dense"], luminance_of=d[:, :32])
        with pytest.raises(ValueError):
            net.inverse_u8(forms["dense"], scratch=scratch)


# ------------------------------------------------------------------------------------------------ the frame loop
H_, W_, N_ = 64, 96, 6


def _style(net, seed=7, hw=(48, 64)):
    return net.forward_u8(_u8(_frames(1, hw[0], hw[1], seed)[0]))


def _run_pipe(pipe, frames, masks=None):
    got = []
    assert pipe.run(frames, lambda i, a: got.append(a.copy()), masks=masks) == len(frames)
    return got


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), (what, i)


@pytest.mark.parametrize("streams", [1, 3])
def test_frame_pipeline_plain(streams):
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    net, cw = _net(), cWCT()
    frames = _frames(N_, H_, W_, 100)
    with torch.no_grad():
        stats = cw.style_stats(_style(net))
        tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
        want = [net.inverse_u8(tf(net.forward_u8(_u8(f)), i), luminance_of=_u8(f))[0].cpu().numpy() for i, f in enumerate(frames)]
        plain = [net.inverse_u8(tf(net.forward_u8(_u8(f)), i))[0].cpu().numpy() for i, f in enumerate(frames)]
    pipe = FramePipeline(net, tf, H_, W_, depth=3, compute_streams=streams, preserve_luminance=True)
    _same(_run_pipe(pipe, frames), want, "luminance")
    _same(_run_pipe(pipe, frames[::-1]), want[::-1], "luminance, slots reused")
    # without the flag: today's frames
    _same(_run_pipe(FramePipeline(net, tf, H_, W_, depth=3, compute_streams=streams), frames), plain, "plain")
    assert not np.array_equal(plain[0], want[0])
    # a decode hook is handed the frame's content slot
    seen = []

    def hook(z, content_u8):
        seen.append((tuple(content_u8.shape), content_u8.dtype))
        return net.inverse_u8(z, luminance_of=content_u8)
    _same(_run_pipe(FramePipeline(net, tf, H_, W_, depth=3, compute_streams=streams, decode=hook, preserve_luminance=True), frames),
          want, "hook")
    assert seen == [((1, H_, W_, 3), torch.uint8)] * N_


@pytest.mark.parametrize("streams", [1, 3])
def test_frame_pipeline_static_masks_and_cross_fade(streams):
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from tests.test_gpu_masks import label_map
    net, cw = _net(), cWCT()
    frames = _frames(N_, H_, W_, 120)
    seg, sty = label_map(H_, W_, [1, 2, 3, 4, 5], 3), label_map(56, 72, [1, 2, 3, 4, 5], 4)
    with torch.no_grad():
        z_s = _style(net, 9, (56, 72))
        plan = cw.bind_style(cw.learn_slots(cw.plan_masks(seg[None], sty[None], (1, 32, H_, W_), z_s.shape, "cuda")), z_s)
        stats2 = [cw.style_stats(_style(net, 7)), cw.style_stats(_style(net, 8, (40, 56)))]
    fade = lambda i: [1.0 - i / (N_ - 1), i / (N_ - 1)]                             # noqa: E731
    for what, tf in (("static 5-label masks", lambda z, i: cw.transfer_with_plan(z, None, plan)),
                     ("two-style cross-fade", lambda z, i: cw.transfer_with_stats(z, stats2, 0.0, alpha_s=fade(i)))):
        with torch.no_grad():
            want = [net.inverse_u8(tf(net.forward_u8(_u8(f)), i), luminance_of=_u8(f))[0].cpu().numpy() for i, f in enumerate(frames)]
            plain = [net.inverse_u8(tf(net.forward_u8(_u8(f)), i))[0].cpu().numpy() for i, f in enumerate(frames)]
        _same(_run_pipe(FramePipeline(net, tf, H_, W_, compute_streams=streams, preserve_luminance=True), frames), want, what)
        _same(_run_pipe(FramePipeline(net, tf, H_, W_, compute_streams=streams), frames), plain, what + ", no flag")
        assert not np.array_equal(want[0], want[-1])


@pytest.mark.parametrize("streams", [1, 3])
def test_frame_pipeline_per_frame_masks_with_a_redone_frame(streams):
    """frame 3 has ten valid labels: it overflows the packed route's 8 slots and is done again on the dense route, which takes
    the Lab step like every other frame"""
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline, MaskSlot
    from tests.test_gpu_masks import clip_maps
    net, cw = _net(), cWCT()
    frames = _frames(N_, H_, W_, 140)
    sty, maps = clip_maps()
    maps = [maps[k] for k in (0, 1, 2, 3, 6, 0)]
    with torch.no_grad():
        binding = cw.bind_style_labels(_style(net, 9, sty.shape), sty)

    def planned(z_c, ms, cap):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(H_, W_, 32, "cuda")
        return cw.transfer_with_plan(z_c, None, cw.plan_frame(ms.mask, binding, max_slots=cap, buffers=buf, flags=ms.flags))
    tf = lambda z, i, ms: planned(z, ms, 8)                                     # noqa: E731
    redo = lambda z, i, ms: planned(z, ms, 32)                                  # noqa: E731
    want, plain, redone = [], [], []
    with torch.no_grad():
        for i, (f, m) in enumerate(zip(frames, maps)):                          # one frame at a time, the flag word read at once
            d = _u8(f)
            ms = MaskSlot(0, torch.zeros(1, dtype=torch.int32, device="cuda"))
            ms.mask = T(m).cuda()
            z = tf(net.forward_u8(d), i, ms)
            if int(ms.flags.item()) & _lib.MASK_OVERFLOW:
                redone.append(i)
                z = redo(net.forward_u8(d), i, ms)
                assert not int(ms.flags.item())
            want.append(net.inverse_u8(z, luminance_of=d)[0].cpu().numpy())
            plain.append(net.inverse_u8(z)[0].cpu().numpy())
    assert redone == [3]
    pipe = FramePipeline(net, tf, H_, W_, compute_streams=streams, redo=redo, preserve_luminance=True)
    _same(_run_pipe(pipe, frames, masks=maps), want, "per-frame masks")
    assert pipe.redo_count == 1
    pipe = FramePipeline(net, tf, H_, W_, compute_streams=streams, redo=redo)
    _same(_run_pipe(pipe, frames, masks=maps), plain, "per-frame masks, no flag")
    assert pipe.redo_count == 1


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("mode", ["host", "device"])
def test_frame_pipeline_writer_size_differs(mode, streams):
    """video_transfer.py's own size context with a writer size that is not the stylised size: the Lab step runs at the
    stylised size, on the float image, and the hook's resize and quantisation follow it"""
    import video_transfer
    from models.cWCT import cWCT
    from vstnet_amd.color import luminance_transfer_u8
    from vstnet_amd.resize import resize_to_u8
    net, cw = _net(), cWCT()
    frames = _frames(N_, H_, W_, 160)
    Ho, Wo = H_ + 24, W_
    with torch.no_grad():
        z_s = _style(net)
        stats = cw.style_stats(z_s)
    outs = {}
    for lum in (True, False):
        args = video_transfer.build_parser().parse_args(["--resize", mode, "--depth", "3", "--streams", str(streams)] +
                                                        (["--preserve_luminance"] if lum else []))
        ctx = video_transfer._SizeContext(args, net, cw, z_s, stats, None, (W_, H_), (Wo, Ho), torch.device("cuda"))
        assert ctx.pipe.preserve_luminance is lum
        got = _run_pipe(ctx.pipe, frames)
        want = []
        with torch.no_grad():
            for f in frames:
                d = _u8(f)
                sty = net(cw.transfer_with_stats(net.forward_u8(d), stats), forward=False)
                if lum:
                    sty = luminance_transfer_u8(d, sty, to_float=True)
                if mode == "device":
                    out = resize_to_u8(sty, (Ho, Wo))
                else:
                    out = F.interpolate(sty, size=(Ho, Wo), mode="bicubic", align_corners=False, antialias=True)
                    out = out.mul(255).clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous()
                want.append(out[0].cpu().numpy())
        assert want[0].shape == (Ho, Wo, 3)
        _same(got, want, (mode, lum))
        outs[lum] = got
    assert not np.array_equal(outs[True][0], outs[False][0])


# ------------------------------------------------------------------------------------------------ the script
def _png(path, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(yy * 3 + seed * 40) % 256, (xx * 2 + seed * 90) % 256, (yy + xx) % 256], -1).astype(np.uint8)
    img = (img.astype(np.int32) + rng.integers(-20, 20, img.shape)).clip(0, 255).astype(np.uint8)
    Image.fromarray(img).save(path)
    return img


def _read(d):
    return [np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))]


def test_video_transfer_script_preserve_luminance(tmp_path):
    import video_transfer
    fd = tmp_path / "clip"
    fd.mkdir()
    n = 5
    frames = [_png(fd / f"{i:03d}.png", 48, 68, 11 + i) for i in range(n)]
    style = _png(tmp_path / "s.png", 40, 40, 3)
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only", "--preserve_luminance"]
    one = _read(video_transfer.main(base + ["--out_dir", str(tmp_path / "one")]))
    assert len(one) == n
    sd = synthetic_state_dict(1234)
    tt = lambda a: T(np.ascontiguousarray(a)).permute(2, 0, 1)[None].float().div(255)      # noqa: E731
    for i in range(n):
        with torch.no_grad():
            sty = cpu_ref.stylize(tt(frames[i]), tt(style), sd, 2)[3]
            ref = cpu_ref.to_uint8(cpu_ref.luminance_transfer(tt(frames[i]), sty))[0].numpy()
        d = np.abs(one[i].astype(int) - ref.astype(int))
        print(f"frame {i}: max diff {d.max()}, differing share {(d > 0).mean():.3e}")
        assert one[i].shape == ref.shape and d.max() <= 1 and (d > 0).mean() < 2e-2, i
    shards = []
    for r in range(2):
        shards += _read(video_transfer.main(base + ["--out_dir", str(tmp_path / f"shard{r}"), "--shard", f"{r}/2"]))
    assert len(shards) == n
    for i in range(n):
        assert np.array_equal(shards[i], one[i]), i
    plain = _read(video_transfer.main([a for a in base if a != "--preserve_luminance"] + ["--out_dir", str(tmp_path / "plain")]))
    assert not np.array_equal(plain[0], one[0])
