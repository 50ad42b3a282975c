"""GPU: the mask producers of csrc/masks.hip (bit-exact against the host functions they replace), per-frame label plans, the
label-keyed factor, and a clip with one label map per frame through video_transfer.py --content_seg_dir --seg_remap."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from vstnet_amd import _lib, masks
from vstnet_amd.synth import synthetic_state_dict, synthetic_frames

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
SIZES = [(64, 96), (36, 52), (1080, 1920)]          # (36, 52): 117 cells (odd), 1872 pixels: no multiple of 16 rows / 64 pixels


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "segremap.npz"))


def make_net(precision=None):
    from models.RevResNet import RevResNet
    net = RevResNet(hidden_dim=16, sp_steps=2, precision=precision)
    sd = synthetic_state_dict(1234, 16, 2)
    net.load_state_dict(sd)
    return net.to("cuda").eval(), sd


def colour_map(h, w, seed):
    """exact dictionary colours, near colours, L1 ties and random colours"""
    from utils.utils import SEG_COLORS
    rng = np.random.default_rng(seed)
    cols = np.array([c for c, _ in SEG_COLORS], dtype=np.int64)
    m = cols[rng.integers(0, 9, (h, w))]
    near = rng.random((h, w)) < 0.3
    m[near] = np.clip(m[near] + rng.integers(-40, 41, (int(near.sum()), 3)), 0, 255)
    ties = np.array([(64, 64, 64), (127, 127, 127), (0, 0, 127), (0, 0, 128), (128, 128, 0), (255, 128, 128), (128, 0, 128),
                     (0, 128, 0), (191, 191, 191), (192, 192, 192), (127, 255, 127)])
    m[0, : len(ties)] = ties
    rnd = rng.random((h, w)) < 0.1
    m[rnd] = rng.integers(0, 256, (int(rnd.sum()), 3))
    return m.astype(np.uint8)


def label_map(h, w, labels, seed, small=()):
    """vertical bands of `labels` with jittered edges; each label of `small` on a few pixels only"""
    rng = np.random.default_rng(seed)
    edges = np.linspace(0, w, len(labels) + 1).astype(int)
    m = np.zeros((h, w), np.uint8)
    for k, l in enumerate(labels):
        m[:, edges[k]: edges[k + 1]] = l
    for k, l in enumerate(small):
        m[2 + 3 * k, 1: 1 + 5 + k] = l
    m[:, :] = np.where(rng.random((h, w)) < 0.02, np.roll(m, 3, axis=1), m)
    return m


# ------------------------------------------------------------------------------------------------ producers, bit-exact
def test_colors_to_labels_matches_the_reference_loop():
    m = colour_map(40, 52, 0)
    want = cpu_ref.colors_to_labels_loop(m)
    got = masks.colors_to_labels(T(m).cuda()).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    from utils.utils import colors_to_labels
    big = colour_map(1080, 1920, 1)
    assert np.array_equal(masks.colors_to_labels(T(big).cuda()).cpu().numpy(), colors_to_labels(big))


def test_device_segremapping_golden(golden):
    from models.segmentation.SegReMapping import SegReMapping
    dev = masks.DeviceSegReMapping(golden["mapping"], float(golden["min_ratio"]))
    host = SegReMapping(golden["mapping"].astype(np.int64), float(golden["min_ratio"]))
    for t in range(int(golden["n_cases"])):
        seg, sty = T(golden[f"seg_{t}"]).cuda(), T(golden[f"sty_{t}"]).cuda()
        a, b = dev.self_remapping(seg), dev.self_remapping(sty)
        assert a.dtype == torch.uint8 and a.is_cuda
        assert np.array_equal(a.cpu().numpy(), golden[f"self_seg_{t}"]) and np.array_equal(b.cpu().numpy(), golden[f"self_sty_{t}"])
        assert np.array_equal(dev.cross_remapping(a, b).cpu().numpy(), golden[f"cross_{t}"])
        assert np.array_equal(dev.cross_remapping(seg, sty).cpu().numpy(), host.cross_remapping(golden[f"seg_{t}"], golden[f"sty_{t}"]))
    dev.check()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_segremapping_random_1080p(golden, seed):
    """4-12 labels, some below min_ratio, half of them absent from the style map"""
    rng = np.random.default_rng(seed)
    labels = [int(l) for l in rng.choice(150, size=int(rng.integers(4, 13)), replace=False)]
    small = [int(l) for l in rng.choice([l for l in range(150) if l not in labels], size=3, replace=False)]
    seg = label_map(1080, 1920, labels, seed, small=small)
    sty = label_map(720, 1280, labels[::2] + small[:1], seed + 10)
    ref = cpu_ref.SegReMappingLoop(golden["mapping"].astype(np.int64), 0.01)
    dev = masks.DeviceSegReMapping(golden["mapping"], 0.01)
    a_ref, s_ref = ref.self_remapping(seg), ref.self_remapping(sty)
    assert (a_ref != seg).any()
    a, s = dev.self_remapping(T(seg).cuda()), dev.self_remapping(T(sty).cuda())
    assert np.array_equal(a.cpu().numpy(), a_ref) and np.array_equal(s.cpu().numpy(), s_ref)
    c_ref = ref.cross_remapping(a_ref, s_ref)
    assert (c_ref != a_ref).any()
    assert np.array_equal(dev.cross_remapping(a, s).cpu().numpy(), c_ref)
    dev.check()


def test_device_segremapping_flags_a_label_outside_the_table(golden):
    seg = np.zeros((40, 40), np.uint8)
    seg[0, :3] = 200
    dev = masks.DeviceSegReMapping(golden["mapping"], 0.01)
    out = dev.self_remapping(T(seg).cuda())
    assert np.array_equal(out.cpu().numpy(), seg)
    with pytest.raises(IndexError):
        dev.check()


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("colours", [False, True])
def test_fused_prepare_matches_mask_to_code_and_bincount(hw, colours):
    from utils.utils import colors_to_labels
    H, W = hw
    L = _lib.lib()
    if colours:
        src = colour_map(H, W, 3)
        lab = colors_to_labels(src)
    else:
        lab = src = np.random.default_rng(4).integers(0, 256, (H, W), dtype=np.uint8) if H < 100 else label_map(H, W, [3, 9, 200, 255, 0], 5)
    d_lab = T(lab).cuda()
    want_rows = torch.empty(H * W, dtype=torch.uint8, device="cuda")
    _lib.check(L.vst_mask_to_code(ptr(d_lab), ptr(want_rows), H, W, stream()), "vst_mask_to_code")
    rows = torch.full((H * W + 64,), 77, dtype=torch.uint8, device="cuda")
    hist = torch.full((256,), -5, dtype=torch.int32, device="cuda")
    _lib.check(L.vst_mask_prepare(ptr(T(src).cuda()), int(colours), H, W, ptr(rows), ptr(hist), stream()), "vst_mask_prepare")
    assert torch.equal(rows[: H * W], want_rows) and bool((rows[H * W:] == 77).all())
    assert np.array_equal(hist.cpu().numpy(), np.bincount(lab.reshape(-1), minlength=256))
    assert np.array_equal(masks.label_hist(d_lab).cpu().numpy(), np.bincount(lab.reshape(-1), minlength=256))


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("cap", [8, 32])
def test_frame_plan_matches_plan_masks_on_host_remapped_maps(golden, hw, cap):
    from models.cWCT import cWCT
    from models.segmentation.SegReMapping import SegReMapping
    H, W = hw
    sH, sW = 40, 56
    labels = [2, 5, 9, 17, 30, 44, 61, 80, 99, 120]
    seg = label_map(H, W, labels, 7, small=[130, 131])
    sty = label_map(sH, sW, labels[:7] + [140], 8)
    host = SegReMapping(golden["mapping"].astype(np.int64), 0.01)
    sty_self = host.self_remapping(sty)
    seg_re = host.cross_remapping(host.self_remapping(seg), sty_self)
    cw = cWCT()
    z_s = torch.randn(1, 32, sH, sW, device="cuda")
    ref_plan = cw.plan_masks(seg_re[None], sty_self[None], (1, 32, H, W), z_s.shape, "cuda")
    ref_labels, _ = cw.plan_info(ref_plan)
    raw = ref_plan.tables[0].cpu().numpy()
    ref_lut = raw[8 + 2048: 8 + 2048 + 256]
    binding = cw.bind_style_labels(z_s, sty_self)
    plan = cw.plan_frame(T(seg).cuda(), binding, remap=masks.DeviceSegReMapping(golden["mapping"], 0.01), max_slots=cap)
    got_labels, over = cw.plan_info(plan)
    tab = plan.tables[0].cpu().numpy()
    lut = tab[8 + 2048: 8 + 2048 + 256]
    assert plan.max_slots == cap and got_labels == ref_labels[:cap] and over == (len(ref_labels) > cap)
    assert int(plan.flags.item()) == (masks.OVERFLOW if len(ref_labels) > cap else 0)
    want_slot = ref_lut[seg_re]
    want_slot = np.where(want_slot >= cap, 255, want_slot)
    assert np.array_equal(lut[seg], want_slot)
    assert np.array_equal(tab[8: 8 + 1024].view(np.int32), np.bincount(seg_re.reshape(-1), minlength=256))
    if cap == 8:
        want_rows = torch.empty(H * W, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib().vst_mask_to_code(ptr(T(seg).cuda()), ptr(want_rows), H, W, stream()), "vst_mask_to_code")
        assert torch.equal(plan.cm_rows[0], want_rows)
    else:
        assert np.array_equal(plan.cm[0].cpu().numpy().reshape(H, W), seg)


def test_label_keyed_factor_is_bit_identical():
    """the same records, once in the content plan's slot order (vst_cwct_factor_labels), once in the style plan's"""
    from models.cWCT import cWCT
    H, W, sH, sW, N = 64, 96, 56, 72, 32
    cw = cWCT()
    L = _lib.lib()
    z_c, z_s = torch.randn(1, N, H, W, device="cuda"), torch.randn(1, N, sH, sW, device="cuda") * 1.5 + 0.3
    seg = label_map(H, W, [4, 9, 20, 33], 1)
    sty = label_map(sH, sW, [1, 4, 9, 12, 20, 33, 50], 2)        # the style has labels the content lacks: the slot orders differ
    binding = cw.bind_style_labels(z_s, sty)
    plan = cw.plan_frame(T(seg).cuda(), binding, max_slots=8)
    labels, _ = cw.plan_info(plan)
    s_raw = binding.plan.cpu().numpy()
    s_lut = s_raw[8 + 2048: 8 + 2048 + 256]
    assert labels == [4, 9, 20, 33] and [int(s_lut[l]) for l in labels] == [1, 2, 4, 5]
    rec = 1 + N + N * N
    cs = cw._stats_labels(z_c.reshape(1, N, -1)[0], T(seg).cuda().reshape(-1), plan.tables[0], 8)
    by_content = torch.zeros_like(binding.stats)
    for k, l in enumerate(labels):
        by_content[k * rec: (k + 1) * rec] = binding.stats[int(s_lut[l]) * rec: (int(s_lut[l]) + 1) * rec]
    out = []
    for keyed in (False, True):
        aff = torch.zeros(32 * (N * N + N), device="cuda")
        info = torch.zeros(32 * 3, dtype=torch.int32, device="cuda")
        if keyed:
            _lib.check(L.vst_cwct_factor_labels_keyed(ptr(cs), ptr(binding.stats), ptr(plan.tables[0]), ptr(binding.plan), 8, 2e-5,
                                                      N, ptr(aff), ptr(info), stream()), "keyed")
        else:
            _lib.check(L.vst_cwct_factor_labels(ptr(cs), ptr(by_content), ptr(plan.tables[0]), 8, 2e-5, N, ptr(aff), ptr(info),
                                                stream()), "factor_labels")
        out.append((aff.cpu(), info.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][0][: 4 * (N * N + N)].abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ the pipeline
class _SyncCounter:
    """counts the host synchronisations torch offers on this code path"""

    def __init__(self, monkeypatch):
        self.n = {}
        for owner, name in ((torch.cuda.Event, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"),
                            (torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy")):
            orig = getattr(owner, name)
            key = f"{getattr(owner, '__name__', owner)}.{name}"
            self.n[key] = 0

            def wrapped(*a, _orig=orig, _key=key, **kw):
                if not (_key == "Tensor.numpy" and not a[0].is_cuda):
                    self.n[_key] += 1
                return _orig(*a, **kw)
            monkeypatch.setattr(owner, name, wrapped)


def test_per_frame_masks_need_no_extra_sync_and_equal_the_static_plan(golden, monkeypatch):
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    H, W, sH, sW, n = 64, 96, 56, 72, 7
    net, _ = make_net()
    cw = cWCT()
    frames = [(synthetic_frames(1, H, W, seed=30 + i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(n)]
    seg = label_map(H, W, [1, 2, 3, 4, 5], 3)
    sty = label_map(sH, sW, [1, 2, 3, 4, 5], 4)
    with torch.no_grad():
        z_s = net.forward_u8((synthetic_frames(1, sH, sW, seed=9).permute(0, 2, 3, 1) * 255).byte().cuda())
        static = cw.bind_style(cw.learn_slots(cw.plan_masks(seg[None], sty[None], (1, 32, H, W), z_s.shape, "cuda")), z_s)
        binding = cw.bind_style_labels(z_s, sty)
    want, got = [], []
    FramePipeline(net, lambda z, i: cw.transfer_with_plan(z, None, static), H, W, compute_streams=3).run(
        frames, lambda i, f: want.append(f.copy()))
    assert cw.last_route == "masked_packed_rows"

    def transform(z_c, i, ms):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, "cuda")
        return cw.transfer_with_plan(z_c, None, cw.plan_frame(ms.mask, binding, max_slots=8, buffers=buf, flags=ms.flags))
    pipe = FramePipeline(net, transform, H, W, compute_streams=3)
    pipe.run(frames[:1], lambda i, f: None, masks=[seg])          # rings and buffers exist before the counted run
    torch.cuda.synchronize()
    counter = _SyncCounter(monkeypatch)
    pipe.run(frames, lambda i, f: got.append(f.copy()), masks=[seg] * n)
    monkeypatch.undo()
    assert cw.last_route == "masked_packed_rows" and pipe.redo_count == 0
    assert counter.n.pop("Event.synchronize") == n, counter.n          # the one done[k].synchronize() per retired frame
    assert not any(counter.n.values()), counter.n
    for a, b in zip(want, got):
        assert np.array_equal(a, b)


def _png(path, h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(yy * 3 + seed * 40) % 256, (xx * 2 + seed * 90) % 256, (yy + xx) % 256], -1).astype(np.uint8)
    img = (img.astype(np.int32) + rng.integers(-20, 20, img.shape)).clip(0, 255).astype(np.uint8)
    Image.fromarray(img).save(path)
    return img


def _bands(h, w, labels):
    edges = np.linspace(0, w, len(labels) + 1).astype(int)
    m = np.zeros((h, w), np.uint8)
    for k, l in enumerate(labels):
        m[:, edges[k]: edges[k + 1]] = l
    return m


def clip_maps():
    """Style 96 x 128: label 3 on the upper 55 rows (7040 pixels), labels 0, 1, 2, 4..10 in bands below.
    Frames 64 x 96 (frame 4: 48 x 80):
      0: labels 0, 1, 2                    1: label 2 has vanished
      2: label 3 on 64 pixels (over 1 % of the frame, so self_remapping leaves it): 7040 > 100 * 64 - it fails the validity
         rule (count ratio), labels 0, 1 stay valid.  The label is kept SMALL on purpose: pixels without a slot pass through
         the network unchanged, come back as the exact integers they were and sit on the knife edge of the reference's
         truncating quantisation, where half of them differ by one between any two implementations
      3: ten valid labels (0, 1, 2, 4..10): more than the packed route's 8 slots - done again on the dense route
      4: another frame size               5: label 60 is absent from the style (cross_remapping), label 12 covers 20 pixels
                                              (self_remapping)
      6: labels 0, 1, 2 again"""
    sty = _bands(96, 128, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10])
    sty[:55] = 3
    f = [_bands(64, 96, [0, 1, 2]), _bands(64, 96, [0, 1])]
    m = _bands(64, 96, [0, 1])
    m[10, 16:80] = 3
    f.append(m)
    f.append(_bands(64, 96, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]))
    f.append(_bands(48, 80, [2, 1, 0]))
    m = _bands(64, 96, [0, 60, 1])
    m[5, 3:23] = 12
    f.append(m)
    f.append(_bands(64, 96, [1, 0, 2]))
    return sty, f


def host_maps(table):
    from models.segmentation.SegReMapping import SegReMapping
    host = SegReMapping(table.astype(np.int64), 0.01)
    sty, frames = clip_maps()
    smask = host.self_remapping(sty)
    return smask, [host.cross_remapping(host.self_remapping(m), smask) for m in frames], frames


def test_clip_maps_give_the_oracle_the_intended_labels(golden):
    """(needs no GPU, kept next to the test that relies on it)"""
    smask, cmasks, raw = host_maps(golden["mapping"])
    assert np.array_equal(smask, clip_maps()[0])                      # the style's self_remapping moves nothing
    valid = []
    for m in cmasks:
        labels, ok = cpu_ref.compute_label_info(m, smask)
        valid.append([int(l) for l in labels if ok[l]])
    assert valid[0] == [0, 1, 2] and valid[1] == [0, 1] and valid[4] == [0, 1, 2] and valid[6] == [0, 1, 2]
    assert int((cmasks[2] == 3).sum()) == 64 and valid[2] == [0, 1]    # present, but not valid
    assert valid[3] == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]
    assert 60 in raw[5] and 12 in raw[5] and 60 not in cmasks[5] and 12 not in cmasks[5] and len(valid[5]) >= 2
    assert sum(len(v) > 8 for v in valid) == 1


@pytest.mark.parametrize("precision", [None, "f16x2h"])
def test_video_transfer_script_per_frame_maps(tmp_path, golden, precision):
    from PIL import Image
    import video_transfer
    fd, sd_ = tmp_path / "clip", tmp_path / "segs"
    fd.mkdir()
    sd_.mkdir()
    smask, cmasks, raw = host_maps(golden["mapping"])
    sty_raw = clip_maps()[0]
    frames = [_png(fd / f"{i:03d}.png", m.shape[0], m.shape[1], 20 + i) for i, m in enumerate(raw)]
    for i, m in enumerate(raw):
        Image.fromarray(m, mode="L").save(sd_ / f"{i:03d}.png")
    style = _png(tmp_path / "s.png", 96, 128, 5)
    Image.fromarray(sty_raw, mode="L").save(tmp_path / "sseg.png")
    np.save(tmp_path / "rel.npy", golden["mapping"])
    args = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--out_dir", str(tmp_path / "o"), "--synthetic_weights",
            "--content_seg_dir", str(sd_), "--style_seg", str(tmp_path / "sseg.png"), "--frames_only", "--seg_remap",
            "--label_mapping", str(tmp_path / "rel.npy")]
    out = video_transfer.main(args + (["--precision", precision] if precision else []))
    names = sorted(os.listdir(out))
    assert names == [f"{i:05d}.png" for i in range(len(raw))]
    assert video_transfer.LAST_RUN["redo"] == 1                           # the frame built to overflow, and only that one
    sd = synthetic_state_dict(1234)
    tt = lambda a: T(np.ascontiguousarray(a)).permute(2, 0, 1)[None].float().div(255)      # noqa: E731
    for i, nme in enumerate(names):
        got = np.asarray(Image.open(os.path.join(out, nme)))
        assert got.shape == (64, 96, 3)
        h, w = frames[i].shape[:2]
        with torch.no_grad():
            sty = cpu_ref.stylize(tt(frames[i]), tt(style), sd, 2, cmasks[i][None], smask[None])[3]
        if (h, w) != (64, 96):
            sty = torch.nn.functional.interpolate(sty, size=(64, 96), mode="bicubic", align_corners=False, antialias=True)
        ref = cpu_ref.to_uint8(sty)[0].numpy()
        d = np.abs(got.astype(int) - ref.astype(int))
        print(f"frame {i}: max diff {d.max()}, differing {(d > 0).mean():.2e}")
        assert d.max() <= 1 and (d > 0).mean() < (1e-2 if precision is None else 5e-2), (i, d.max(), (d > 0).mean())
