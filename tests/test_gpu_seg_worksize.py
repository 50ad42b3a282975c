"""Segmenting at a working resolution (segment_u8(work_size=...), --seg_size) against the fp64 goldens of
tests/make_segformer_worksize_golden.py, and the two logits -> labels samplers against each other.

Bounds.  The label comparison is the one of tests/test_gpu_segformer.py, unchanged: the device may be 8 x e32 off (e32 = the
reference's own fp32 error on the working frame, recorded per case), labels must agree wherever the fp64 top-2 margin exceeds
twice that, and at least 99 % of the pixels must be decided.  The samplers are compared for EXACT equality (they share taps,
weights and the four-term sum), and with fp64 F.interpolate + argmax wherever the fp64 margin exceeds 1e-4 of max |logit|: an
fp32 coordinate (error ~ 40 * 2^-24 at these sizes) and four fp32 products move a sampled value by ~1e-5 of max |logit|.
Every test prints its counts before it asserts (-s)."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from vstnet_amd.synth import synthetic_scene_u8, synthetic_segformer_state_dict, synthetic_state_dict

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 4321
FACTOR = 8
CASES = {"up4": (288, 416), "ragged": (283, 409), "chain": (144, 208), "same": (96, 136)}
TILE_H, TILE_W = 16, 64            # csrc/segformer.hip UP_TH, UP_TW


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "segformer_worksize.npz")))


@pytest.fixture(scope="module")
def models():
    from vstnet_amd.segformer import SegFormer
    cache = {}

    def get(depths):
        depths = tuple(int(d) for d in depths)
        if depths not in cache:
            cache[depths] = SegFormer(depths=depths).load_state_dict(synthetic_segformer_state_dict(SEED, depths))
        return cache[depths]
    return get


def case_frame(golden, case):
    h, w = CASES[case]
    frame = synthetic_scene_u8(h, w, int(golden[f"{case}.scene_seed"]))
    assert zlib.crc32(frame.tobytes()) == int(golden[f"{case}.frame_crc32"])
    return frame


def labels_from_logits(lg, H, W, kernel):
    """lg: float32 [Hq, Wq, 150] on the device -> uint8 [H, W] through vst_seg_labels_from_logits."""
    from vstnet_amd import _lib
    assert lg.is_contiguous() and lg.dtype == torch.float32 and lg.shape[2] == 150
    out = torch.empty((H, W), dtype=torch.uint8, device=lg.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().vst_seg_labels_from_logits(C.c_void_p(lg.data_ptr()), int(lg.shape[0]), int(lg.shape[1]), H, W, kernel,
                                                     C.c_void_p(out.data_ptr()), st), "vst_seg_labels_from_logits")
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_labels_at_a_working_resolution(golden, models, case):
    seg = models(golden[f"{case}.depths"])
    frame = torch.from_numpy(case_frame(golden, case)).cuda()
    size = int(golden[f"{case}.work_size"])
    e32, scale = float(golden[f"{case}.e32"]), float(golden[f"{case}.max_logit"])
    labels = seg.segment_u8(frame, work_size=size).cpu().numpy()
    want = golden[f"{case}.labels"]
    decided = golden[f"{case}.margin"].astype(np.float64) > 2 * FACTOR * e32 * scale
    wrong = int(((labels != want) & decided).sum())
    print(f"{case}: {int((labels != want).sum())} labels differ, {wrong} of them decided; {100 * (1 - decided.mean()):.4f} % undecided")
    assert labels.shape == want.shape and labels.dtype == np.uint8
    assert decided.mean() >= 0.99
    assert wrong == 0


def test_a_work_size_that_does_not_shrink_is_the_plain_route(golden, models):
    seg = models(golden["same.depths"])
    frame = torch.from_numpy(case_frame(golden, "same")).cuda()
    plain = seg.segment_u8(frame)
    assert torch.equal(seg.segment_u8(frame, work_size=int(golden["same.work_size"])), plain)
    assert torch.equal(seg.segment_u8(frame, work_size=4096), plain)
    assert torch.equal(seg.segment_work_u8(frame, (96, 136)), plain)


@pytest.mark.parametrize("case", ["up4", "ragged"])
def test_host_resized_upload_gives_the_same_labels(golden, models, case):
    seg = models(golden[f"{case}.depths"])
    frame = case_frame(golden, case)
    h, w = frame.shape[:2]
    size = int(golden[f"{case}.work_size"])
    hw, ww = seg.work_hw(h, w, size)
    work = np.asarray(Image.fromarray(frame).resize((ww, hw), Image.BICUBIC))
    dev = seg.segment_u8(torch.from_numpy(frame).cuda(), work_size=size)
    assert torch.equal(seg.segment_work_u8(torch.from_numpy(work).cuda(), (h, w)), dev)
    # the caller's buffers and a planar frame change nothing
    buf, out = torch.empty(hw * ww * 3 + 5, dtype=torch.uint8, device="cuda"), torch.empty((h, w), dtype=torch.uint8, device="cuda")
    assert seg.segment_u8(torch.from_numpy(frame).cuda(), out=out, work_size=size, work=buf) is out and torch.equal(out, dev)
    assert torch.equal(seg.segment_u8(torch.from_numpy(frame).cuda().permute(2, 0, 1).contiguous(), work_size=size), dev)


def plant_ties(lg, H, W):
    """Exact ties between two and three classes (0 and 149 among them), above everything else, in 2 x 2 cell blocks in the four
    corners and in the cells around the first tile seams.  Returns [(y, x, expected label)] for pixels inside the blocks."""
    Hq, Wq = lg.shape[:2]
    g = torch.Generator().manual_seed(7)

    def plant(cys, cxs, classes):
        for cy in cys:
            for cx in cxs:
                lg[cy, cx, list(classes)] = 8.0 + float(torch.rand((), generator=g))
    plant((0, 1), (0, 1), (0, 149))
    plant((0, 1), (Wq - 2, Wq - 1), (149, 7, 0))
    plant((Hq - 2, Hq - 1), (0, 1), (3, 149))
    plant((Hq - 2, Hq - 1), (Wq - 2, Wq - 1), (148, 149))
    expect = [(0, 0, 0), (0, W - 1, 0), (H - 1, 0, 3), (H - 1, W - 1, 148)]

    def seam_cell(tile, cells, pixels):         # the cell under the first tile seam that is clear of the corner blocks
        for p in range(tile, pixels, tile):
            if 3 <= p * cells // pixels <= cells - 4:
                return p * cells // pixels
        return None
    cy, cx = seam_cell(TILE_H, Hq, H), seam_cell(TILE_W, Wq, W)
    if cy is not None and cx is not None:
        plant(range(cy - 1, cy + 2), range(cx - 1, cx + 2), (75, 0, 149))
    return expect


@pytest.mark.parametrize("shape", [(8, 8, 32, 32), (18, 26, 283, 409), (9, 13, 577, 97), (24, 34, 96, 136), (8, 40, 640, 161)])
def test_tiled_sampler_equals_the_per_pixel_sampler(shape):
    Hq, Wq, H, W = shape
    lg = torch.randn((Hq, Wq, 150), generator=torch.Generator().manual_seed(Hq * 1000 + Wq), dtype=torch.float32)

    def reference(t):
        full = F.interpolate(t.cuda().double().permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False)[0]
        top = full.topk(2, dim=0)
        return top.indices[0].to(torch.uint8), (top.values[0] - top.values[1]) > 1e-4 * float(t.abs().max())
    for planted in (False, True):
        expect = plant_ties(lg, H, W) if planted else []
        d = lg.cuda().contiguous()
        k0, k1 = labels_from_logits(d, H, W, 0), labels_from_logits(d, H, W, 1)
        want, decided = reference(lg)
        share = float(decided.float().mean())
        wrong = int(((k1 != want) & decided).sum())
        print(f"{shape} planted={planted}: kernels differ on {int((k0 != k1).sum())} pixels; {wrong} decided pixels differ from fp64; "
              f"{100 * (1 - share):.4f} % undecided")
        if not planted:
            assert share >= 0.99           # plain Gaussian logits: the reference itself leaves under 1 % of the pixels close
        assert torch.equal(k0, k1)
        assert wrong == 0
        for y, x, label in expect:
            assert int(k1[y, x]) == label, (y, x, int(k1[y, x]), label)
    assert torch.equal(labels_from_logits(d, H, W, -1), k0)


def test_large_map_with_64_bit_pixel_offsets(models):
    """16384 x 16400 labels from a 32 x 32 working frame (an 8 x 8 logit grid): the run's dispatch against the per-pixel sampler
    on the same logits.  The map has 2^28 + 262,144 pixels, i.e. 269 MB: no byte offset of it reaches 2^31, so the middle band
    straddles the largest power of two inside it, pixel 2^28.  (The device compares the whole maps too; that takes no longer.)"""
    H, W = 16384, 16400
    seg = models((1, 1, 1, 1))
    work = torch.from_numpy(synthetic_scene_u8(32, 32, 9)).cuda()
    lg = seg.logits(work)[0].permute(1, 2, 0).contiguous()
    assert tuple(lg.shape) == (8, 8, 150)
    got = seg.segment_work_u8(work, (H, W))
    tiled, want = labels_from_logits(lg, H, W, 1), labels_from_logits(lg, H, W, 0)
    mid = (1 << 28) // W
    for lo, hi in ((0, 16), (mid - 8, mid + 8), (H - 16, H)):
        a, b, c = got[lo:hi].cpu().numpy(), want[lo:hi].cpu().numpy(), tiled[lo:hi].cpu().numpy()
        print(f"rows {lo}..{hi}: {int((a != b).sum())} / {int((c != b).sum())} pixels differ, {len(np.unique(b))} labels")
        assert np.array_equal(a, b) and np.array_equal(c, b)
    assert torch.equal(got, want) and torch.equal(tiled, want)
    assert int(torch.unique(want[::64, ::64]).numel()) >= 2


def test_side_stream_with_another_work_size_frame_in_flight(golden, models):
    seg = models(golden["up4.depths"])
    big = torch.from_numpy(case_frame(golden, "up4")).cuda()
    small = torch.from_numpy(case_frame(golden, "ragged")).cuda()
    alone_small, alone_big = seg.segment_u8(small, work_size=101).clone(), seg.segment_u8(big, work_size=104).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        got_big = seg.segment_u8(big, work_size=104)                  # in flight on the current stream
        with torch.cuda.stream(side):
            got_small = seg.segment_u8(small, work_size=101)
    torch.cuda.synchronize()
    assert torch.equal(got_small, alone_small) and torch.equal(got_big, alone_big)


def test_errors(models):
    from vstnet_amd import _lib
    from vstnet_amd.segformer import MAX_LABEL_PIXELS
    seg = models((1, 1, 1, 1))
    frame = torch.zeros((64, 96, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="32"):
        seg.segment_u8(frame, work_size=31)
    with pytest.raises(ValueError, match="--seg_size"):               # 1024 -> 32 is a 32 x shrink
        seg.segment_u8(torch.zeros((1024, 64, 3), dtype=torch.uint8, device="cuda"), work_size=32)
    # a label map above the limit: VST_E_SHAPE before anything is launched (the label buffer is never touched)
    tiny = torch.zeros(16, dtype=torch.uint8, device="cuda")
    work = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda")
    H, W = 1 << 15, (1 << 15) + 1
    assert H * W > MAX_LABEL_PIXELS
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().vst_seg_run_scaled_u8(seg._plan, C.c_void_p(work.data_ptr()), 0, 32, 32, H, W, C.c_void_p(tiny.data_ptr()), st)
    assert rc == -2
    with pytest.raises(_lib.VstError, match="-2"):
        _lib.check(rc, "vst_seg_run_scaled_u8")
    lg = torch.zeros((8, 8, 150), dtype=torch.float32, device="cuda")
    for kernel in (0, 1, -1):
        assert _lib.lib().vst_seg_labels_from_logits(C.c_void_p(lg.data_ptr()), 8, 8, H, W, kernel, C.c_void_p(tiny.data_ptr()), st) == -2
    # a working frame under 32 pixels on an edge, and the tiled sampler where its tile does not fit (no upsampling)
    assert _lib.lib().vst_seg_run_scaled_u8(seg._plan, C.c_void_p(work.data_ptr()), 0, 31, 32, 64, 64, C.c_void_p(tiny.data_ptr()), st) == -2
    big = torch.zeros((64, 64, 150), dtype=torch.float32, device="cuda")
    out = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    assert _lib.lib().vst_seg_labels_from_logits(C.c_void_p(big.data_ptr()), 64, 64, 64, 64, 1, C.c_void_p(out.data_ptr()), st) == -2
    torch.cuda.synchronize()
    assert int(tiny.sum()) == 0


def test_frame_pipeline_with_a_working_resolution_equals_uploaded_maps(models):
    """Three 144 x 208 frames: FramePipeline(seg_work_size=104) against the per-frame mask route fed, from the host, the maps
    segment_u8(..., work_size=104) returned for the same frames."""
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    H, W, S = 144, 208, 104
    seg = models((1, 1, 1, 1))
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234, 16, 2))
    net = net.to("cuda").eval()
    cw = cWCT()
    frames = [synthetic_scene_u8(H, W, 10 + i) for i in range(3)]
    style = synthetic_scene_u8(64, 88, 20)
    maps = [seg.segment_u8(torch.from_numpy(f).cuda(), work_size=S).cpu().numpy() for f in frames]
    plain = seg.segment_u8(torch.from_numpy(frames[0]).cuda()).cpu().numpy()
    assert not np.array_equal(maps[0], plain)                   # (the working resolution is a different segmentation)
    sty = seg.segment_u8(torch.from_numpy(style).cuda()).cpu().numpy()
    with torch.no_grad():
        binding = cw.bind_style_labels(net.forward_u8(torch.from_numpy(style)[None].cuda()), sty)

    def plan(ms, cap):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, "cuda")
        return cw.plan_frame(ms.mask, binding, max_slots=cap, buffers=buf, flags=ms.flags)

    def transform(z_c, i, ms):
        return cw.transfer_with_plan(z_c, None, plan(ms, 8))

    def redo(z_c, i, ms):
        return cw.transfer_with_plan(z_c, None, plan(ms, 32))
    want, got, seen = [], [], []
    FramePipeline(net, transform, H, W, redo=redo).run(frames, lambda i, f: want.append(f.copy()), masks=maps)
    pipe = FramePipeline(net, transform, H, W, redo=redo, segmenter=seg, seg_work_size=S, mask_sink=lambda i, m: seen.append(m.copy()))
    pipe.run(frames, lambda i, f: got.append(f.copy()))
    assert len(got) == 3 and len(seen) == 3
    for a, b, f, m, s in zip(want, got, frames, maps, seen):
        assert np.array_equal(m, s)
        assert np.array_equal(a, b)
        assert not np.array_equal(b, f)
    with pytest.raises(ValueError, match="segmenter"):
        FramePipeline(net, transform, H, W, seg_work_size=S)
