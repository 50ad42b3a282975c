"""The temporal logit window of --auto_seg video (--seg_window, DESIGN.md "Temporal window") on the GPU: the mixing kernel
against the same chain of fp32 torch operations (exact), the labels of mixed logits against fp64, FramePipeline(seg_window=...)
against a serial restatement (also under a working resolution, a decay and warm-up frames), and video_transfer.py with shards.

Bounds.  The mix is compared for EXACT equality: the kernel computes w0 * x0, then + w1 * x1, ... with every product and sum
rounded to fp32 and no fused multiply-add, which is what separate torch multiplies and adds compute.  Labels are compared with
fp64 (weighted mean, F.interpolate, argmax) wherever the fp64 top-2 margin exceeds 1e-4 of max |mean logit|, the bound
tests/test_gpu_seg_worksize.py uses for the samplers alone: the mix adds at most n * 2^-24 relative error to a value the sampler
moves by ~1e-5.  At most 1 % of the pixels may be undecided.  The counts are printed before they are asserted (-s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from vstnet_amd.synth import SEG_DEPTHS, synthetic_scene_u8, synthetic_segformer_state_dict, synthetic_state_dict

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 64, 96
N_FRAMES = 7


@pytest.fixture(scope="module")
def seg():
    from vstnet_amd.segformer import SegFormer
    return SegFormer("b1", embedding_dim=256).load_state_dict(synthetic_segformer_state_dict(4321, SEG_DEPTHS["b1"], 256))


@pytest.fixture(scope="module")
def net():
    from models.RevResNet import RevResNet
    n = RevResNet(hidden_dim=16, sp_steps=2)
    n.load_state_dict(synthetic_state_dict(1234, 16, 2))
    return n.to("cuda").eval()


@pytest.fixture(scope="module")
def frames():
    return [synthetic_scene_u8(H, W, 40 + i) for i in range(N_FRAMES)]


def torch_mix(xs, w):
    """The kernel's chain with separate fp32 torch operations on the device: one rounding per product and per sum."""
    acc = xs[0] * float(w[0])
    for x, wk in zip(xs[1:], w[1:]):
        acc = acc + x * float(wk)
    return acc


def labels_from_logits(lg, grid, out_hw, kernel=-1):
    from vstnet_amd import _lib
    out = torch.empty(out_hw, dtype=torch.uint8, device=lg.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().vst_seg_labels_from_logits(C.c_void_p(lg.data_ptr()), grid[0], grid[1], out_hw[0], out_hw[1], kernel,
                                                     C.c_void_p(out.data_ptr()), st), "vst_seg_labels_from_logits")
    return out


@pytest.fixture(scope="module")
def serial(seg, frames):
    """(work_size, decay) -> the maps a window of 3 gives the clip, one frame at a time: seg.logits of each frame, the torch mix,
    vst_seg_labels_from_logits.  Computed once per key."""
    from vstnet_amd.resize import resize_u8
    from vstnet_amd.segformer import window_weights
    cache = {}

    def get(work_size=None, decay=1.0, window=3):
        key = (work_size, decay, window)
        if key not in cache:
            lgs, maps = [], []
            for f in frames:
                d = torch.from_numpy(f).cuda()
                hw, ww = seg.work_hw(H, W, work_size)
                if (hw, ww) != (H, W):
                    d = resize_u8(d, (ww, hw))
                lg = seg.logits(d)[0].permute(1, 2, 0).contiguous()          # [Hq, Wq, 150], token-major
                lgs.append(lg)
                n = min(window, len(lgs))
                mixed = torch_mix(lgs[::-1][:n], window_weights(n, decay)).contiguous()
                maps.append(labels_from_logits(mixed, tuple(lg.shape[:2]), (H, W)).cpu().numpy())
            cache[key] = maps
        return cache[key]
    return get


# ------------------------------------------------------------------------------------------------------------- 1. the mix, exact
# 150: one cell (a tail of two floats behind 37 float4); 9*13*150 and 16*16*150: logit grids; 1050: not a multiple of 4 * 256;
# 150 * 14000 = 2,100,000 floats: more float4 than the grid's 2048 * 256 threads, so the grid-stride loop goes round
@pytest.mark.parametrize("count", [150, 9 * 13 * 150, 16 * 16 * 150, 1050, 150 * 14000])
def test_mix_equals_the_torch_chain(seg, count):
    g = torch.Generator().manual_seed(count)
    xs = [torch.randn(count, generator=g).cuda() for _ in range(8)]
    w_all = torch.rand(8, generator=g).numpy().astype(np.float32) + np.float32(0.05)
    for n in range(1, 9):
        out = torch.full((count,), 7.0, device="cuda")
        seg.mix_logits(xs[:n], w_all[:n], out)
        assert torch.equal(out, torch_mix(xs[:n], w_all[:n])), n
    out = torch.full((count,), 7.0, device="cuda")
    seg.mix_logits(xs[:1], [1.0], out)
    assert torch.equal(out.view(torch.int32), xs[0].view(torch.int32))       # n = 1, w = 1: a bit copy


def test_mix_of_pointers_that_are_only_8_byte_aligned(seg):
    """Views two floats into their buffers: 8-byte but not 16-byte aligned, the float2 form of the kernel."""
    count = 9 * 13 * 150
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(count + 2, generator=g).cuda()[2:] for _ in range(3)]
    w = np.array([0.5, 0.3, 0.2], np.float32)
    assert all(x.data_ptr() % 16 == 8 for x in xs)
    for out in (torch.zeros(count, device="cuda"), torch.zeros(count + 2, device="cuda")[2:]):
        seg.mix_logits(xs, w, out)
        assert torch.equal(out, torch_mix(xs, w))


# ------------------------------------------------------------------------------------------------------- 2. labels against fp64
@pytest.mark.parametrize("grid, out_hw, n, decay", [((9, 13), (70, 101), 4, 1.0), ((8, 8), (250, 250), 8, 0.7),
                                                    ((12, 20), (48, 80), 1, 1.0)])
def test_labels_of_mixed_logits_against_fp64(seg, grid, out_hw, n, decay):
    from vstnet_amd.segformer import window_weights
    g = torch.Generator().manual_seed(grid[0] * 1000 + grid[1] + n)
    base = torch.randn((grid[0], grid[1], 150), generator=g)
    xs = [(base + 0.5 * torch.randn(base.shape, generator=g)).cuda().reshape(-1, 150).contiguous() for _ in range(n)]
    w = window_weights(n, decay)
    mean = sum(float(wk) * x.double() for wk, x in zip(w, xs)).reshape(grid[0], grid[1], 150)
    full = F.interpolate(mean.permute(2, 0, 1)[None], size=out_hw, mode="bilinear", align_corners=False)[0]
    top = full.topk(2, dim=0)
    want, decided = top.indices[0].to(torch.uint8), (top.values[0] - top.values[1]) > 1e-4 * float(mean.abs().max())
    mixed = seg.mix_logits(xs, w, torch.empty_like(xs[0]))
    kernels = (-1, 1) if out_hw[0] >= 4 * grid[0] and out_hw[1] >= 4 * grid[1] else (-1,)      # (1: the tiled sampler, where it fits)
    for kernel in kernels:
        got = seg.labels_from_logits(mixed, grid, out_hw) if kernel < 0 else labels_from_logits(mixed, grid, out_hw, kernel)
        wrong, undecided = int(((got != want) & decided).sum()), 1.0 - float(decided.float().mean())
        print(f"{grid}->{out_hw} n={n} kernel={kernel}: {int((got != want).sum())} labels differ, {wrong} of them decided; "
              f"{100 * undecided:.4f} % undecided")
        assert undecided <= 0.01
        assert wrong == 0


# -------------------------------------------------------------------------------------------- 3.-5. the pipeline against serial
def run_pipeline(net, seg, clip, start=0, warmup=(), **kw):
    """The label maps FramePipeline hands its mask_sink, {frame index: map}.  The transform leaves the code alone: the maps are
    what is compared here, the masked transfer on top of them is test_video_transfer_seg_window's."""
    from vstnet_amd.pipeline import FramePipeline
    seen = {}
    pipe = FramePipeline(net, lambda z, i, ms: z, H, W, segmenter=seg, compute_streams=3, depth=4,
                         mask_sink=lambda i, m: seen.__setitem__(i, m.copy()), **kw)
    n = pipe.run(clip, lambda i, f: None, start_index=start, warmup=warmup)
    assert n == len(clip) and sorted(seen) == list(range(start, start + n))
    return pipe, seen


@pytest.mark.parametrize("work_size, decay", [(None, 1.0), (48, 1.0), (None, 0.5)])
def test_pipeline_equals_serial(net, seg, frames, serial, work_size, decay):
    pipe, seen = run_pipeline(net, seg, frames, seg_window=3, seg_work_size=work_size, seg_decay=decay)
    want = serial(work_size, decay)
    assert pipe.logit_ring is not None and pipe.logit_ring.shape[0] == 3 + 4
    for i in range(N_FRAMES):
        assert np.array_equal(seen[i], want[i]), i
    assert not np.array_equal(want[2], serial(work_size, 1.0, window=1)[2])        # (the window does change the maps)
    if (work_size, decay) != (None, 1.0):
        assert any(not np.array_equal(a, b) for a, b in zip(want, serial(None, 1.0)))


def test_window_1_is_the_per_frame_route(net, seg, frames):
    pipe, seen = run_pipeline(net, seg, frames, seg_window=1)
    assert pipe.logit_ring is None and pipe.logit_mix is None
    for i, f in enumerate(frames):
        assert np.array_equal(seen[i], seg.segment_u8(torch.from_numpy(f).cuda()).cpu().numpy()), i
    with pytest.raises(ValueError, match="warmup"):
        pipe.run(frames[1:], lambda i, f: None, start_index=1, warmup=frames[:1])
    with pytest.raises(ValueError, match="segmenter"):
        from vstnet_amd.pipeline import FramePipeline
        FramePipeline(net, lambda z, i: z, H, W, seg_window=3)


def test_warmup_frames_give_a_shard_the_full_runs_maps(net, seg, frames, serial):
    want = serial(None, 1.0)
    _, seen = run_pipeline(net, seg, frames[3:], start=3, warmup=frames[1:3], seg_window=3)
    for i in range(3, N_FRAMES):
        assert np.array_equal(seen[i], want[i]), i
    _, cold = run_pipeline(net, seg, frames[3:], start=3, seg_window=3)
    assert not np.array_equal(cold[3], want[3]) and not np.array_equal(cold[4], want[4])     # the window started over
    for i in range(5, N_FRAMES):                                                             # ... and has filled by frame 5
        assert np.array_equal(cold[i], want[i]), i


# ------------------------------------------------------------------------------------------------------------------ 6. scripts
def test_video_transfer_seg_window_and_two_shards(tmp_path, frames, serial):
    import video_transfer
    fd = tmp_path / "clip"
    fd.mkdir()
    for i, f in enumerate(frames[:6]):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
    Image.fromarray(synthetic_scene_u8(72, 104, 50)).save(tmp_path / "s.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only", "--auto_seg",
            "--synthetic_seg_weights", "--seg_variant", "b1", "--no_seg_remap", "--seg_window", "3"]
    one = video_transfer.main(base + ["--out_dir", str(tmp_path / "o1")])
    names = ["%05d.png" % i for i in range(6)]
    assert sorted(os.listdir(one)) == names
    want = serial(None, 1.0)
    for i in range(6):
        got = np.asarray(Image.open(tmp_path / "o1" / "segmentation" / ("%05d_label.png" % i)))
        assert np.array_equal(got, want[i]), i
    assert video_transfer.LAST_RUN["flicker"] == pytest.approx(
        np.mean([np.mean(want[i] != want[i + 1]) for i in range(5)]), abs=1e-12)
    # the two shards one after the other, each in a fresh process with its own time limit
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    for shard in ("0/2", "1/2"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py")] + base
                           + ["--out_dir", str(tmp_path / "o2"), "--shard", shard], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (shard, r.stderr[-3000:])
    two = os.path.join(str(tmp_path / "o2"), os.path.basename(one))
    assert sorted(os.listdir(two)) == names
    for i, n in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(os.path.join(one, n))), np.asarray(Image.open(os.path.join(two, n)))), n
        a, b = (tmp_path / o / "segmentation" / ("%05d_label.png" % i) for o in ("o1", "o2"))
        assert np.array_equal(np.asarray(Image.open(a)), np.asarray(Image.open(b))), i


# ------------------------------------------------------------------------------------------------------------------- 7. errors
def test_mix_errors_launch_nothing():
    from vstnet_amd import _lib
    L, vp = _lib.lib(), C.c_void_p
    count = 300
    buf = torch.ones(2 * count + 8, device="cuda")
    xs = [torch.ones(count, device="cuda") for _ in range(8)]
    out = torch.zeros(count, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    w = (C.c_float * 8)(*[0.5] * 8)
    ptrs = (vp * 8)(*[x.data_ptr() for x in xs])

    def call(p=ptrs, wt=w, n=2, c=count, o=out.data_ptr()):
        return L.vst_seg_mix_logits(p, wt, n, c, vp(o), st)
    assert call(p=None) == -1 and call(wt=None) == -1 and call(o=0) == -1
    assert call(p=(vp * 2)(xs[0].data_ptr(), 0)) == -1                                   # a null input
    assert call(p=(vp * 2)(xs[0].data_ptr(), xs[1].data_ptr() + 4)) == -1                # a misaligned input
    assert call(o=out.data_ptr() + 4) == -1                                              # a misaligned out
    assert call(p=(vp * 2)(xs[0].data_ptr(), out.data_ptr())) == -1                      # out is an input
    assert call(p=(vp * 2)(buf.data_ptr(), xs[1].data_ptr()), o=buf.data_ptr() + 4 * (count - 2)) == -1      # out overlaps one
    for n in (0, 9):
        assert call(n=n) == -2
    for c in (0, 151, (1 << 20) * 150 + 2):
        assert call(c=c) == -2
    with pytest.raises(_lib.VstError, match="-2"):
        _lib.check(call(n=9), "vst_seg_mix_logits")
    torch.cuda.synchronize()
    assert int(out.count_nonzero()) == 0 and float(buf.min()) == 1.0 == float(buf.max())
    assert call() == 0                                                                   # and the same call, valid, runs
    torch.cuda.synchronize()
    assert float(out.min()) == 1.0 == float(out.max())
