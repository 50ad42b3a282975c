"""The deep resize on the GPU ("Deep resize"; include/vstnet.h): vst_yuv16_img_resize_f32 against the float64
reference within the tolerance tests/deep_resize_ref.py derives (fp32 roundings only), on planes from one flat buffer - odd sizes
put U and V on odd 2-byte addresses - with every byte around the outputs guarded; the u8 twin EQUAL to floor(255 v + 0.5) of the
stored float output, every sample; the single call against DeepImgResize; a conforming size against yuv16_to_rgb_f32; and
FramePipeline with src_deep_resize=True bit-identical to the same library calls made one frame at a time; video_transfer.py
--resize device on a deep clip above --max_size."""
import numpy as np
import pytest
import torch

import deep_resize_ref as R
from deep_resize_ref import DeepYuvSpec
from vstnet_amd.synth import synthetic_state_dict
from vstnet_amd.yuv import DeepImgResize, rgb_f32_to_yuv16, rgb_to_yuv16_host, yuv16_img_resize_f32, yuv16_to_rgb_f32

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5

# the four layouts at depth 10, 4:2:0-left at depths 9, 12 and 16; both matrices and both ranges are in the set
SPECS = [DeepYuvSpec("444", "bt601", "full", 10), DeepYuvSpec("422", "bt709", "limited", 10),
         DeepYuvSpec("420jpeg", "bt601", "limited", 10), DeepYuvSpec("420mpeg2", "bt709", "full", 10),
         DeepYuvSpec("420mpeg2", "bt709", "limited", 9), DeepYuvSpec("420mpeg2", "bt601", "full", 12),
         DeepYuvSpec("420mpeg2", "bt709", "limited", 16)]


class Guarded:
    """a device buffer of `nbytes` with 256 sentinel bytes on either side, `shift` bytes off the 256-byte grid"""

    def __init__(self, nbytes, shift=0):
        self.lo, self.n = 256 + shift, nbytes
        self.buf = torch.full((self.lo + nbytes + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[self.lo:self.lo + nbytes]

    def check(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:self.lo] == SENTINEL).all() and (host[self.lo + self.n:] == SENTINEL).all(), \
            f"{what}: bytes outside the output were written"
        return host[self.lo:self.lo + self.n].copy()


def resize_case(spec, Ws, Hs, max_size, seed):
    """one frame through yuv16_img_resize_f32 on outputs off and on the 16-byte grid and without the twin; returns the largest
    error over the tolerance"""
    what = f"{spec} {Ws}x{Hs} to {max_size}"
    flat = R.random_planes(spec, Hs, Ws, seed)
    w, h = R.img_resize_size((Ws, Hs), max_size, R.DOWN_SCALE)
    src = Guarded(flat.size, 2)                 # (the flat frame starts 2 bytes off the grid)
    src.view.copy_(torch.from_numpy(flat))
    f, b = Guarded(12 * h * w, 4), Guarded(3 * h * w, 1)         # (off the 16-byte grid: the narrow paths)
    out = yuv16_img_resize_f32(src.view, Hs, Ws, spec, max_size, R.DOWN_SCALE, out=f.view.view(torch.float32).view(1, 3, h, w),
                               out_u8=b.view.view(h, w, 3))
    assert out.data_ptr() == f.view.data_ptr() and tuple(out.shape) == (1, 3, h, w)
    fa, ba = Guarded(12 * h * w), Guarded(3 * h * w)            # (on the grid: the 16-byte paths)
    yuv16_img_resize_f32(src.view, Hs, Ws, spec, max_size, R.DOWN_SCALE, out=fa.view.view(torch.float32).view(1, 3, h, w),
                         out_u8=ba.view.view(h, w, 3))
    f2 = Guarded(12 * h * w, 4)
    yuv16_img_resize_f32(src.view, Hs, Ws, spec, max_size, R.DOWN_SCALE, out=f2.view.view(torch.float32).view(1, 3, h, w))
    torch.cuda.synchronize()
    got = f.check(what).view(np.float32).reshape(3, h, w)
    twin = b.check(what).reshape(h, w, 3)
    assert np.array_equal(f2.check(what + ", no twin").view(np.float32).reshape(3, h, w), got), what + ": the twin changes the floats"
    assert np.array_equal(fa.check(what + ", aligned").view(np.float32).reshape(3, h, w), got), what + ": alignment changes the floats"
    assert np.array_equal(ba.check(what + ", aligned").reshape(h, w, 3), twin), what + ": alignment changes the twin"
    assert np.array_equal(src.check(what + ", source"), flat)
    want = R.reference(flat, Hs, Ws, spec, max_size)
    assert want.shape == (h, w, 3)
    err = float(np.abs(got.transpose(1, 2, 0).astype(np.float64) - want).max())
    tol = R.kernel_tolerance((Ws, Hs), max_size)
    print(f"{what}: largest error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, f"{what}: {err:.3e} from the float64 reference, tolerance {tol:.3e}"
    assert got.min() >= 0.0 and got.max() <= 1.0
    bad = twin != R.twin_of(got.transpose(1, 2, 0))
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes of the twin differ from floor(255 v + 0.5) of the float output"
    return err / tol


@pytest.mark.parametrize("spec", SPECS, ids=repr)
def test_kernel_against_float64(spec):
    for n, (Ws, Hs, max_size) in enumerate(R.SHAPES):
        resize_case(spec, Ws, Hs, max_size, 100 * spec.depth + n)


def test_single_call_equals_the_per_slot_object():
    spec = SPECS[2]
    for Ws, Hs, max_size in R.SHAPES:
        d = torch.from_numpy(R.random_planes(spec, Hs, Ws, 5)).cuda()
        rs = DeepImgResize((Hs, Ws), spec, max_size, R.DOWN_SCALE, "cuda")
        w, h = rs.size_wh
        u1, u2 = (torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        a = yuv16_img_resize_f32(d, Hs, Ws, spec, max_size, R.DOWN_SCALE, out_u8=u1)
        b = rs(d, out_u8=u2)
        c = rs(spec.split(d, Hs, Ws))          # (the object again, on the planes: its buffers are reused)
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(u1, u2), (Ws, Hs, max_size)


def test_a_conforming_size_is_the_conversion():
    spec, Hs, Ws = SPECS[3], 56, 40
    d = torch.from_numpy(R.random_planes(spec, Hs, Ws, 9)).cuda()
    u1, u2 = (torch.empty((Hs, Ws, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    rs = DeepImgResize((Hs, Ws), spec, 64, R.DOWN_SCALE, "cuda")
    assert rs.steps == [(Ws, Hs)] and rs.tables is None and rs.work is None
    assert torch.equal(rs(d, out_u8=u1), yuv16_to_rgb_f32(d, Hs, Ws, spec, out_u8=u2)) and torch.equal(u1, u2)


def test_argument_errors_on_device_tensors():
    from vstnet_amd import _lib
    spec = DeepYuvSpec()
    with pytest.raises(_lib.VstError, match="16"):
        DeepImgResize((64, 2000), spec, 64, 4, "cuda")         # 2000 -> 64: a shrink of 31
    rs = DeepImgResize((80, 112), spec, 56, 4, "cuda")
    flat = torch.zeros(spec.frame_bytes(80, 112), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        rs(flat[:-2])
    with pytest.raises(ValueError):
        rs(flat, out=torch.zeros((1, 3, 40, 60), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        rs(flat, out_u8=torch.zeros((40, 60, 3), dtype=torch.uint8, device="cuda"))


# --------------------------------------------------------------------------------------------------------------- the pipeline
HS_, WS_, H_, W_, MAX_, N_ = 80, 112, 40, 56, 56, 4
DEEP_IN, DEEP_OUT = DeepYuvSpec("420mpeg2", "bt709", "limited", 10), DeepYuvSpec("422", "bt709", "full", 12)


@pytest.fixture(scope="module")
def net():
    from models.RevResNet import RevResNet
    n = RevResNet(hidden_dim=16, sp_steps=2)
    n.load_state_dict(synthetic_state_dict(1234, 16, 2))
    return n.to("cuda").eval()


@pytest.fixture(scope="module")
def cw():
    from models.cWCT import cWCT
    return cWCT()


@pytest.fixture(scope="module")
def s_stats(net, cw):
    from vstnet_amd.synth import synthetic_scene_u8
    with torch.no_grad():
        return cw.style_stats(net.forward_u8(torch.from_numpy(synthetic_scene_u8(48, 64, 77)).cuda()[None]))


def deep_frame(seed):
    """a source-size frame's bytes of a smooth synthetic scene with a fractional part (codes off the multiples of 4)"""
    from vstnet_amd.synth import synthetic_scene_u8
    rgb = (synthetic_scene_u8(HS_, WS_, seed).astype(np.float64) + np.random.default_rng(seed).uniform(0, 1, (HS_, WS_, 3))) / 256.0
    return rgb_to_yuv16_host(rgb, DEEP_IN)


def serial(net, cw, s_stats, frames, lum, out, out_hw):
    """one stream, one frame at a time, the library calls the pipeline is documented to make"""
    from vstnet_amd.color import luminance_transfer
    from vstnet_amd.resize import resize_f32
    rs, outs = DeepImgResize((HS_, WS_), DEEP_IN, MAX_, 4, "cuda"), []
    with torch.no_grad():
        for f in frames:
            u8 = torch.empty((1, H_, W_, 3), dtype=torch.uint8, device="cuda")
            x = rs(torch.from_numpy(f).cuda(), out_u8=u8)
            z_cs = cw.transfer_with_stats(net(x), s_stats)
            if out is None:
                outs.append(net.inverse_u8(z_cs, luminance_of=u8 if lum else None)[0].cpu().numpy())
                continue
            sty = net._inverse(z_cs)
            if lum:
                sty = luminance_transfer(x, sty)
            if out_hw is not None:
                sty = resize_f32(sty, out_hw)
            outs.append(rgb_f32_to_yuv16(sty, out).cpu().numpy())
    return outs


def run(pipe, frames):
    got = {}
    assert pipe.run(frames, lambda i, a: got.__setitem__(i, a.copy())) == len(frames)
    return [got[i] for i in sorted(got)]


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (what, i)


@pytest.mark.parametrize("mode", ["plain", "luminance", "deep out at another size"])
def test_pipeline_equals_the_calls_one_frame_at_a_time(net, cw, s_stats, mode):
    """4 source-size frames through 3 slots on 2 streams, so a slot is reused; then a second run of the same pipeline, reversed"""
    from vstnet_amd.pipeline import FramePipeline
    frames = [deep_frame(500 + i) for i in range(N_)]
    lum = mode == "luminance"
    out, out_hw = (DEEP_OUT, (60, 84)) if mode.startswith("deep out") else (None, None)
    kw = dict(out_yuv=out, out_height=out_hw[0], out_width=out_hw[1]) if out is not None else {}
    pipe = FramePipeline(net, lambda z, i, **k: cw.transfer_with_stats(z, s_stats, **k), H_, W_, depth=3, compute_streams=2,
                         src_yuv=DEEP_IN, src_height=HS_, src_width=WS_, max_size=MAX_, src_deep_resize=True,
                         preserve_luminance=lum, **kw)
    assert tuple(pipe.h_in.shape) == (3, DEEP_IN.frame_bytes(HS_, WS_)) and tuple(pipe.d_xf.shape) == (3, 1, 3, H_, W_)
    want = serial(net, cw, s_stats, frames, lum, out, out_hw)
    same(run(pipe, frames), want, mode)
    same(run(pipe, frames[::-1]), serial(net, cw, s_stats, frames[::-1], lum, out, out_hw), mode + ", a second run")
    assert len({w.tobytes() for w in want}) == N_


def test_pipeline_needs_the_keyword(net, cw, s_stats):
    from vstnet_amd.pipeline import FramePipeline
    tf = lambda z, i: cw.transfer_with_stats(z, s_stats)                           # noqa: E731
    with pytest.raises(ValueError, match="src_deep_resize"):
        FramePipeline(net, tf, H_, W_, src_yuv=DEEP_IN, src_height=HS_, src_width=WS_, max_size=MAX_)
    with pytest.raises(ValueError, match="resizes to"):
        FramePipeline(net, tf, H_, W_ + 4, src_yuv=DEEP_IN, src_height=HS_, src_width=WS_, max_size=MAX_, src_deep_resize=True)


# ----------------------------------------------------------------------------------------------------------------- the script
def test_script_with_resize_device_equals_the_pipeline(tmp_path):
    """video_transfer.py --resize device on a deep clip above --max_size: the bytes of a FramePipeline made by hand.  The writer
    size rule writes this landscape clip at 56x56, not at the stylised 56x40: the pipeline's resize_f32 is part of both sides."""
    import video_transfer
    from image_transfer import build_network
    from models.cWCT import cWCT
    from PIL import Image
    from utils.utils import img_resize, to_tensor_u8
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_scene_u8
    frames = [deep_frame(600 + i) for i in range(3)]
    R.write_raw(str(tmp_path / "clip.yuv"), frames)
    Image.fromarray(synthetic_scene_u8(48, 64, 77)).save(tmp_path / "s.png")
    wsz = video_transfer.writer_size((WS_, HS_), MAX_)
    out = video_transfer.main(["--video", str(tmp_path / "clip.yuv"), "--pix_fmt", "yuv420p10le", "--video_size", "%dx%d" % (WS_, HS_),
                               "--yuv_matrix", "bt709", "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--max_size",
                               str(MAX_), "--resize", "device", "--out_dir", str(tmp_path / "o")])
    assert out == str(tmp_path / "o" / ("clip_s_%dx%d_yuv420p10le.yuv" % wsz))
    net = build_network("photorealistic", None, True, torch.device("cuda"), None)
    cw_ = cWCT()
    with torch.no_grad():
        z_s = net.forward_u8(to_tensor_u8(img_resize(Image.open(tmp_path / "s.png").convert("RGB"), MAX_, down_scale=4)).cuda())
        stats = cw_.style_stats(z_s)
    pipe = FramePipeline(net, lambda z, i: cw_.transfer_with_stats(z, stats), H_, W_, src_yuv=DEEP_IN, out_yuv=DEEP_IN,
                         out_height=wsz[1], out_width=wsz[0], src_height=HS_, src_width=WS_, max_size=MAX_, src_deep_resize=True)
    want = run(pipe, frames)
    assert open(out, "rb").read() == b"".join(w.tobytes() for w in want) and len({w.tobytes() for w in want}) == 3
