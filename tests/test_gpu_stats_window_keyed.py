"""The statistics window by label (--stats_by_label, DESIGN.md section 5 "Statistics window by label") on the GPU:
vst_cwct_stats_pool_keyed against a long-double truth over named key patterns, its bits against the unkeyed kernel's, the window
through the real per-label statistics kernels against fp64 statistics of each label's pixels over the frames, FramePipeline(
stats_by_label=True) against a serial restatement (plan ring deeper than the frame ring, warm-up frames, one map for the whole
clip, a frame with more than 8 labels), video_transfer.py with shards, and the refusals.

Bounds.  Kernel: device <= 4 x max(e64, 2^-53) under the statistics metrics with the pooled C (tests/stats_window_ref.py), e64 =
the keyed fp64 restatement (tests/stats_window_keyed_ref.py) against the same long-double truth; `used` equal; records under the
copy rule equal as bits; records of dead slots unwritten.  Through the statistics kernels: FACTOR['stats'] x max(e32, U) of
tests/cwct_ops_ref.py, e32 = stats_labels32 per frame pooled by the keyed restatement.  Pipelines and shards: byte equality.
The figures are printed before they are asserted (-s)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import cwct_ops_ref as O
import stats_window_keyed_ref as K
import stats_window_ref as R
from vstnet_amd.synth import synthetic_mask, synthetic_scene_u8, synthetic_state_dict

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 64, 96
SH, SW = 72, 104
N_FRAMES = 7
NAN64 = float("nan")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def cw():
    from models.cWCT import cWCT
    return cWCT()


@pytest.fixture(scope="module")
def net():
    from models.RevResNet import RevResNet
    n = RevResNet(hidden_dim=16, sp_steps=2)
    n.load_state_dict(synthetic_state_dict(1234, 16, 2))
    return n.to("cuda").eval()


@pytest.fixture(scope="module")
def frames():
    return [synthetic_scene_u8(H, W, 60 + i) for i in range(N_FRAMES)]


def bands(h, w, labels):
    """vertical bands of equal width, one per label, in the order given"""
    edges = np.linspace(0, w, len(labels) + 1).astype(int)
    m = np.zeros((h, w), np.uint8)
    for k, v in enumerate(labels):
        m[:, edges[k]:edges[k + 1]] = v
    return m


STYLE_LABELS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
# the clip's maps: the label sets differ from frame to frame, so a label's slot does too (0 comes and goes: label 5 is slot 2, 1,
# 2, 1 ...); label 9 is in every second frame only
CLIP_LABELS = [[0, 3, 5], [3, 5, 9], [0, 3, 5, 7], [5, 3, 9], [0, 5, 7], [3, 5, 0, 9], [5, 7, 3]]


@pytest.fixture(scope="module")
def style(net, cw):
    """(binding of the 12-label style map, its code): every label of the clip's maps is valid against it"""
    with torch.no_grad():
        z_s = net.forward_u8(torch.from_numpy(synthetic_scene_u8(SH, SW, 77)).cuda()[None])
        return cw.bind_style_labels(z_s, bands(SH, SW, STYLE_LABELS)), z_s


@pytest.fixture(scope="module")
def clip_maps():
    return [bands(H, W, lab) for lab in CLIP_LABELS]


# ------------------------------------------------------------------------------------------------ (a) the kernel against truth
class Margins:
    """`count` doubles at an offset of one double (8-byte, not 16-byte aligned) inside a buffer filled with `fill`"""

    def __init__(self, shape, fill, pad=3):
        n = int(np.prod(shape))
        self.buf = torch.full((1 + n + pad,), fill, dtype=torch.float64, device="cuda")
        self.view = self.buf[1:1 + n].view(*shape)
        self.n, self.fill = n, fill
        assert self.view.data_ptr() % 16 == 8 and self.view.is_contiguous()

    def margins_untouched(self):
        b = self.buf.cpu().numpy()
        edge = np.concatenate([b[:1], b[1 + self.n:]])
        return bits(edge).tobytes() == bits(np.full_like(edge, self.fill)).tobytes()


# every width of the unkeyed table at 8 slots, and at 32 slots up to N = 128 (the widest records, N = 256, stay at 8 slots, as the
# unkeyed table keeps its wide records at R <= 8: 32 of them are 17 MB per age and say nothing that N = 128 does not)
KERNEL_CASES = [(N, ms, p) for N in R.WIDTHS for ms in (8, 32) if ms == 8 or N <= 128
                for p in list(K.KEY_PATTERNS) + ["cut_one_label"]]


@pytest.mark.parametrize("N,ms,pattern", KERNEL_CASES, ids=lambda v: str(v))
def test_keyed_kernel_against_truth(cw, N, ms, pattern):
    cut_label = pattern == "cut_one_label"
    pattern_in = "reversed_older" if cut_label else pattern
    records, labels, weights, cut = K.keyed_input(N, ms, pattern_in, cut_label=cut_label)
    raw_plans = K.keyed_plans(pattern_in, ms, labels)
    truth, used = K.pool_keyed_ref(records, labels, weights, cut, np.longdouble)
    r64, used64 = K.pool_keyed_ref(records, labels, weights, cut)
    n0 = len(labels[0])
    assert np.array_equal(used, used64) and not used[n0:].any()
    if cut_label:
        assert used[0] == 1 and set(used[1:n0]) == {3}
    if pattern == "missing_middle":
        assert used[1] == 2 and set(np.delete(used[:n0], 1)) == {3}          # the age is skipped, the scan goes on
    if pattern == "missing_everywhere":
        assert used[0] == 1 and set(used[1:n0]) == {3}
    if pattern == "empty_older":                                             # (n_slots = 0 over stale labels and valid records)
        assert set(used[:n0]) == {2} and labels[0][0] == 0 and K.plan_labels(raw_plans[2]) == []
        assert list(raw_plans[2][K.PLAN_LABELS:K.PLAN_LABELS + n0]) == labels[0] and (records[2][:n0, 0] >= 2).all()
    if pattern == "short_newest":
        assert n0 < ms and set(used[:n0]) == {3}
    if pattern == "label_zero":                                              # (age 1's padding is zero and must not match)
        assert labels[0][0] == 0 and used[0] == 2 and (records[1][len(labels[1]):, 0] >= 2).all()
    if pattern in ("label_zero", "empty_older"):       # a lookup past n_slots finds a valid record here: the inputs can tell
        _, loose = K.pool_keyed_ref(records, labels, weights, cut, plans=raw_plans, mut=("unbounded_search",))
        assert not np.array_equal(loose, used)
    ins = [Margins(r.shape, NAN64) for r in records]
    for m, r in zip(ins, records):
        m.view.copy_(torch.from_numpy(r))
    plans = [torch.from_numpy(p).cuda() for p in raw_plans]
    out = Margins(records[0].shape, O.SENTINEL_F64)
    d_used = torch.full((ms + 2,), -7, dtype=torch.int32, device="cuda")
    got_t = cw.pool_stats([m.view for m in ins], weights=weights, cut=cut, out=out.view, used=d_used[1:1 + ms], plans=plans)
    assert got_t.data_ptr() == out.view.data_ptr()
    got, got_used = out.view.cpu().numpy(), d_used.cpu().numpy()
    ratio, (gc, gm, ec, em) = R.pool_ratio(got[:n0], r64[:n0], truth[:n0], used[:n0], N)
    print(f"keyed pool N={N} slots={ms} {pattern}: e64 cov {ec:.3g} mean {em:.3g}, device cov {gc:.3g} mean {gm:.3g} = {ratio:.2f} x, "
          f"bound {R.FACTOR}")
    assert np.array_equal(got_used[1:1 + ms], used) and got_used[0] == -7 == got_used[-1]
    for r in range(n0):
        if used[r] <= 1:                                   # the copy rule: the bits of the age-0 record
            assert bits(got[r]).tobytes() == bits(records[0][r]).tobytes(), r
    # a dead slot's record is not written
    assert bits(got[n0:]).tobytes() == bits(np.full_like(got[n0:], O.SENTINEL_F64)).tobytes()
    assert out.margins_untouched() and all(m.margins_untouched() for m in ins)
    for m, r, p, raw in zip(ins, records, plans, raw_plans):  # (the inputs are only read)
        assert bits(m.view.cpu().numpy()).tobytes() == bits(r).tobytes()
        assert np.array_equal(p.cpu().numpy(), raw)
    assert ratio <= R.FACTOR, (N, ms, pattern, ratio)


# ------------------------------------------------------------------------------------------------------------ (b) exactness
@pytest.mark.parametrize("N,ms", [(1, 8), (7, 32), (32, 8), (32, 32), (128, 8)])
@pytest.mark.parametrize("cut_label", [False, True])
def test_keyed_bits_equal_the_unkeyed_kernels(cw, N, ms, cut_label):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    for pattern in ("identity", "reversed_older", "missing_middle", "label_zero", "empty_older"):
        records, labels, weights, cut = K.keyed_input(N, ms, pattern, cut_label=cut_label, seed=3)
        n0 = len(labels[0])
        used_k = torch.full((ms,), -7, dtype=torch.int32, device="cuda")
        got = cw.pool_stats([dev(r) for r in records], weights=weights, cut=cut, used=used_k,
                            plans=[dev(p) for p in K.keyed_plans(pattern, ms, labels)]).cpu().numpy()
        # identity keys: the unkeyed kernel on the very same blocks; otherwise on the blocks gathered by label on the host
        blocks = records if pattern == "identity" else K.gather(records, labels)[0]
        used_u = torch.full((n0,), -7, dtype=torch.int32, device="cuda")
        want = cw.pool_stats([dev(b[:n0]) for b in blocks], weights=weights, cut=cut, used=used_u).cpu().numpy()
        assert np.array_equal(used_k.cpu().numpy()[:n0], used_u.cpu().numpy()), pattern
        assert not used_k.cpu().numpy()[n0:].any()
        assert bits(got[:n0]).tobytes() == bits(want).tobytes(), pattern


# ----------------------------------------------------------------------------------- (c) through the real statistics kernels
def test_window_through_the_per_label_statistics(cw):
    from vstnet_amd.code import from_dense
    masks = [synthetic_mask(H, W, labels=n, seed=s) for n, s in ((5, 3), (4, 8), (5, 13))]      # oldest first
    masks[1] = np.where(masks[1] == 1, 2, masks[1]).astype(np.uint8)      # label 1 is absent from the middle frame
    sseg = synthetic_mask(48, 64, labels=5, seed=4)
    z_s = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 32, 48, 64)).astype(np.float32)).cuda()
    binding = cw.bind_style_labels(z_s, sseg)
    y, x = O.row_pixels(H, W, 2)
    L, per = O.labels_code_groups(H, W)
    recs, tabs, r32, cols, mrows, labels = [], [], [], [], [], []
    for f, m in enumerate(masks):
        z = O.stats_input(32, H * W, "scales", seed=11 + f).reshape(32, H, W)
        code = from_dense(torch.from_numpy(z)[None].cuda())
        plan = cw.plan_frame(torch.from_numpy(m).cuda(), binding, max_slots=8)
        out = torch.full((O.MAX_SLOTS, O.rec_len(32)), O.SENTINEL_F64, dtype=torch.float64, device="cuda")
        assert cw.frame_stats(code, plan, out=out, by_label=True) is out
        raw = plan.tables[0].cpu().numpy()
        lut, lab = raw[8 + 2048:8 + 2048 + 256].copy(), K.plan_labels(raw)
        assert lab == O.plan_ref(m, sseg)[1] and not raw[4:8].view(np.int32)[0]
        rows = code.packed.cpu().numpy().reshape(-1, 32)
        cols.append(np.ascontiguousarray(rows.T))
        mrows.append(m[y, x])
        r32.append(O.stats_labels32(cols[-1], mrows[-1], lut, len(lab), 8, groups=(-(-L // per), per, "code")))
        recs.append(out)
        tabs.append(plan.tables[0].clone())
        labels.append(lab)
    assert labels[2] == [0, 1, 2, 3, 4] and 1 not in labels[1] and 4 not in labels[1] and labels[0] == [0, 1, 2, 3, 4]
    const = int(np.nonzero((rows == O.CONST_VAL).all(0))[0][0])
    used = torch.full((O.MAX_SLOTS,), -7, dtype=torch.int32, device="cuda")
    got = cw.pool_stats(recs[::-1], used=used, plans=tabs[::-1]).cpu().numpy()
    p32, u32 = K.pool_keyed_ref([np.where(r == O.SENTINEL_F64, 0.0, r) for r in r32[::-1]], labels[::-1], np.ones(3), 0.0)
    assert np.array_equal(used.cpu().numpy(), u32) and u32[:5].tolist() == [3, 2, 3, 3, 2] and not u32[5:].any()
    worst = 0.0
    for s, v in enumerate(labels[2]):
        held = [f for f in range(3) if v in labels[f]]
        want = O.stats64(np.concatenate([cols[f][:, mrows[f] == v] for f in held], axis=1))
        assert got[s, 0] == want[0], ("count", v)
        r, (gc, gm, ec, em) = O.stats_ratio(got[s], p32[s], want, 32, skip=(const,))
        print(f"label {v} over frames {held}: e32 cov {ec / O.U:.3g} u mean {em / O.U:.3g} u, device cov {gc / O.U:.3g} u mean "
              f"{gm / O.U:.3g} u = {r:.2f} x, bound {O.FACTOR['stats']}")
        worst = max(worst, r)
    assert worst <= O.FACTOR["stats"]


# --------------------------------------------------------------------------------------- (d)-(f) the pipeline against serial
def per_frame_transforms(cw, binding):
    def buffers(ms):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, "cuda")
        return buf

    def transform(z_c, i, ms, content_stats=None):
        plan = cw.plan_frame(ms.mask, binding, max_slots=8, buffers=buffers(ms), flags=ms.flags)
        kw = {} if content_stats is None else dict(content_stats=content_stats, by_label=True)
        return cw.transfer_with_plan(z_c, None, plan, **kw)

    def redo(z_c, i, ms):
        return cw.transfer_with_plan(z_c, None, cw.plan_frame(ms.mask, binding, max_slots=32, buffers=buffers(ms), flags=ms.flags))
    return transform, redo


def run_pipeline(net, cw, binding, clip, maps, start=0, warmup=(), warmup_masks=None, depth=3, streams=2, **kw):
    from vstnet_amd.pipeline import FramePipeline
    seen = {}
    transform, redo = per_frame_transforms(cw, binding)
    pipe = FramePipeline(net, transform, H, W, depth=depth, compute_streams=streams, redo=redo, **kw)
    more = {} if warmup_masks is None else dict(warmup_masks=warmup_masks)
    n = pipe.run(clip, lambda i, f: seen.__setitem__(i, f.copy()), start_index=start, masks=maps, warmup=warmup, **more)
    assert n == len(clip) and sorted(seen) == list(range(start, start + n))
    return pipe, seen


def run_serial(net, cw, binding, clip, maps, window, decay=1.0, cut=0.0):
    """One stream, one frame at a time, through the library calls: the window is a list of (record, plan table) clones, the pool
    cWCT.pool_stats(plans=...), and a frame whose flag word says overflow is done again on the dense route from its own
    statistics while its cap-8 record and plan stay in the list.  -> (frames, frames pooled per slot and frame, redone)"""
    from vstnet_amd import _lib
    ring, outs, useds, redone = [], [], [], []
    with torch.no_grad():
        for i, (f, m) in enumerate(zip(clip, maps)):
            z = net.forward_u8(torch.from_numpy(f).cuda()[None])
            d_m = torch.from_numpy(m).cuda()
            used = torch.zeros(32, dtype=torch.int32, device="cuda")

            def window_of(rec, b, table):
                ring.insert(0, (rec.clone(), table.clone()))
                del ring[window:]
                return cw.pool_stats([r for r, _ in ring], decay=decay, cut=cut, used=used, plans=[t for _, t in ring])
            plan = cw.plan_frame(d_m, binding, max_slots=8)
            z_cs = cw.transfer_with_plan(z, None, plan, content_stats=window_of, by_label=True)
            if int(plan.flags.cpu()[0]) & _lib.MASK_OVERFLOW:
                z_cs = cw.transfer_with_plan(z, None, cw.plan_frame(d_m, binding, max_slots=32))
                redone.append(i)
            outs.append(net.inverse_u8(z_cs)[0].cpu().numpy())
            useds.append(used.cpu().numpy())
    return outs, useds, redone


@pytest.fixture(scope="module")
def serial(net, cw, frames, style, clip_maps):
    """the W = 4 and W = 2 serial frames of the clip, computed once"""
    return {w: run_serial(net, cw, style[0], frames, clip_maps, w, 0.5) for w in (2, 4)}


@pytest.mark.parametrize("window,depth", [(2, 4), (4, 2)])
def test_pipeline_with_masks_equals_serial(net, cw, frames, style, clip_maps, serial, window, depth):
    """(4, 2): W - 1 > depth, so a pool that read the frames' own plan buffers would see overwritten plans."""
    want, useds, redone = serial[window]
    assert not redone
    pipe, seen = run_pipeline(net, cw, style[0], frames, clip_maps, depth=depth, stats_window=window, stats_decay=0.5,
                              stats_by_label=True)
    assert cw.last_route == "masked_packed_rows" and pipe.redo_count == 0
    assert tuple(pipe.stat_ring.shape) == (window + depth, 32, O.rec_len(32))
    assert tuple(pipe.plan_ring.shape) == (window + depth, K.PLAN_BYTES) and tuple(pipe.h_used.shape) == (depth, 32)
    for i in range(N_FRAMES):
        assert np.array_equal(seen[i], want[i]), i
        live = useds[i][useds[i] > 0]
        assert pipe.window_used[i] == (int(live.min()), min(window, i + 1)), i
    assert pipe.pooled_labels == sum(int((u > 0).sum()) for u in useds)
    assert pipe.pooled_frames == sum(int(u.sum()) for u in useds)
    # label 9 is in every second frame only: at W = 2 it never pools anything, at W = 4 it does
    nine = [int(useds[i][sorted(CLIP_LABELS[i]).index(9)]) for i in (1, 3, 5)]
    assert nine == ([1, 1, 1] if window == 2 else [1, 2, 2])
    plain, _, _ = run_serial(net, cw, style[0], frames[:3], clip_maps[:3], 1)
    assert np.array_equal(plain[0], want[0]) and not np.array_equal(plain[2], want[2])      # (the window does change the frames)


def test_warmup_frames_give_a_shard_the_full_runs_frames(net, cw, frames, style, clip_maps, serial):
    want = serial[4][0]
    _, seen = run_pipeline(net, cw, style[0], frames[4:], clip_maps[4:], start=4, warmup=frames[1:4], warmup_masks=clip_maps[1:4],
                           depth=2, stats_window=4, stats_decay=0.5, stats_by_label=True)
    for i in range(4, N_FRAMES):
        assert np.array_equal(seen[i], want[i]), i
    _, cold = run_pipeline(net, cw, style[0], frames[4:], clip_maps[4:], start=4, depth=2, stats_window=4, stats_decay=0.5,
                           stats_by_label=True)
    assert not np.array_equal(cold[4], want[4])              # the window started over


def test_one_map_for_every_frame_equals_the_static_plan(net, cw, frames, style):
    from vstnet_amd.pipeline import FramePipeline
    binding, z_s = style
    seg, sseg = bands(H, W, [0, 3, 5, 7, 9]), bands(SH, SW, STYLE_LABELS)
    clip = frames[:5]
    static = cw.bind_style(cw.learn_slots(cw.plan_masks(seg[None], sseg[None], (1, 32, H, W), tuple(z_s.shape), "cuda")), z_s)
    assert static.max_slots == 5
    want = {}
    FramePipeline(net, lambda z, i, **k: cw.transfer_with_plan(z, None, static, **k), H, W, depth=3, stats_window=3, stats_decay=0.5,
                  frame_stats=lambda z, out=None: cw.frame_stats(z, static, out=out)).run(
        clip, lambda i, f: want.__setitem__(i, f.copy()))
    pipe, seen = run_pipeline(net, cw, binding, clip, [seg] * 5, stats_window=3, stats_decay=0.5, stats_by_label=True)
    for i in range(5):
        assert np.array_equal(seen[i], want[i]), i
    assert [pipe.window_used[i] for i in range(5)] == [(1, 1), (2, 2), (3, 3), (3, 3), (3, 3)]
    one, _ = run_pipeline(net, cw, binding, clip[:2], [seg] * 2, stats_window=1)
    assert getattr(one, "stat_ring", None) is None and one.stat_window is None and not hasattr(one, "plan_ring")


def test_overflow_frame_is_redone_and_its_record_stays(net, cw, frames, style, clip_maps):
    """Frame 2 has ten valid labels: done again on the dense route from its own statistics (its W = 1 result), counted once;
    its cap-8 record and plan stay in the window of the frames after it."""
    maps = list(clip_maps[:6])
    maps[2] = bands(H, W, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
    clip = frames[:6]
    want, useds, redone = run_serial(net, cw, style[0], clip, maps, 3, 0.5)
    assert redone == [2]
    pipe, seen = run_pipeline(net, cw, style[0], clip, maps, depth=2, stats_window=3, stats_decay=0.5, stats_by_label=True)
    assert pipe.redo_count == 1
    own, _, _ = run_serial(net, cw, style[0], clip[2:3], maps[2:3], 1)
    assert np.array_equal(seen[2], own[0]) and np.array_equal(seen[2], want[2])
    for i in range(6):
        assert np.array_equal(seen[i], want[i]), i
    # frame 3 (labels 3, 5, 9): 3 and 5 are among the first 8 labels of frame 2 and pool it; 9 is past its cap and skips it
    assert useds[3][:3].tolist() == [3, 3, 2]


# ---------------------------------------------------------------------------------------------------------- (g) script shards
def _one_and_two_shards(tmp_path, base, n):
    import video_transfer
    one = video_transfer.main(base + ["--out_dir", str(tmp_path / "o1")])
    names = ["%05d.png" % i for i in range(n)]
    assert sorted(os.listdir(one)) == names
    print("frames pooled per live label:", video_transfer.LAST_RUN["stats_pooled"])
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    for shard in ("0/2", "1/2"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py")] + base
                           + ["--out_dir", str(tmp_path / "o2"), "--shard", shard], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (shard, r.stderr[-3000:])
        assert "statistics window by label" in r.stdout
    two = os.path.join(str(tmp_path / "o2"), os.path.basename(one))
    assert sorted(os.listdir(two)) == names
    for nme in names:
        assert np.array_equal(np.asarray(Image.open(os.path.join(one, nme))), np.asarray(Image.open(os.path.join(two, nme)))), nme
    return one, names


def _write_clip(tmp_path, frames, n=6):
    fd = tmp_path / "clip"
    fd.mkdir()
    for i, f in enumerate(frames[:n]):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
    Image.fromarray(synthetic_scene_u8(SH, SW, 50)).save(tmp_path / "s.png")
    return ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only"]


def test_video_transfer_content_seg_dir_and_two_shards(tmp_path, frames, clip_maps):
    import video_transfer
    base = _write_clip(tmp_path, frames)
    sd = tmp_path / "segs"
    sd.mkdir()
    for i, m in enumerate(clip_maps[:6]):
        Image.fromarray(m, mode="L").save(sd / f"{i:03d}.png")
    Image.fromarray(bands(SH, SW, STYLE_LABELS), mode="L").save(tmp_path / "sseg.png")
    maps = ["--content_seg_dir", str(sd), "--style_seg", str(tmp_path / "sseg.png")]
    one, names = _one_and_two_shards(tmp_path, base + maps + ["--stats_window", "3", "--stats_by_label"], 6)
    # (the last call of this process was the one-process run) labels 3 and 5 are in nearly every frame: more than one frame each
    assert video_transfer.LAST_RUN["stats_pooled"] > 1.5
    plain = video_transfer.main(base + maps + ["--out_dir", str(tmp_path / "o0")])
    differ = [not np.array_equal(np.asarray(Image.open(os.path.join(one, n))), np.asarray(Image.open(os.path.join(plain, n))))
              for n in names]
    assert not differ[0] and all(differ[1:])                 # the flag reaches the frames


def test_video_transfer_auto_seg_both_windows_and_two_shards(tmp_path, frames):
    base = _write_clip(tmp_path, frames)
    _one_and_two_shards(tmp_path, base + ["--auto_seg", "--synthetic_seg_weights", "--seg_variant", "b1", "--no_seg_remap",
                                          "--seg_window", "2", "--stats_window", "3", "--stats_by_label"], 6)


# ------------------------------------------------------------------------------------------------------------------ (h) guards
def test_guards(net, cw, frames, style, clip_maps):
    from vstnet_amd.pipeline import FramePipeline
    binding, z_s = style
    with torch.no_grad():
        z = net.forward_u8(torch.from_numpy(frames[0]).cuda()[None])
    seg, sseg = bands(H, W, [0, 3, 5]), bands(SH, SW, STYLE_LABELS)
    static = cw.bind_style(cw.learn_slots(cw.plan_masks(seg[None], sseg[None], (1, 32, H, W), tuple(z_s.shape), "cuda")), z_s)
    keep = lambda rec, b, table=None: rec      # noqa: E731
    sentinel = torch.full((32, O.rec_len(32)), O.SENTINEL_F64, dtype=torch.float64, device="cuda")
    untouched = lambda: bits(sentinel.cpu().numpy()).tobytes() == bits(np.full((32, O.rec_len(32)), O.SENTINEL_F64)).tobytes()  # noqa: E731
    with pytest.raises(ValueError, match="by_label"):                       # a static plan
        cw.frame_stats(z, static, out=sentinel, by_label=True)
    with pytest.raises(ValueError, match="by_label"):
        cw.frame_stats(z, None, by_label=True)
    with pytest.raises(ValueError, match="by_label"):
        cw.transfer_with_plan(z, None, static, content_stats=keep, by_label=True)
    d_m = torch.from_numpy(clip_maps[0]).cuda()
    dense = cw.plan_frame(d_m, binding, max_slots=32)
    with pytest.raises(NotImplementedError, match="packed route"):          # a dense per-frame plan
        cw.frame_stats(z, dense, out=sentinel, by_label=True)
    per_frame = cw.plan_frame(d_m, binding, max_slots=8)
    with pytest.raises(ValueError, match="static plan"):                    # without the keyword: as before
        cw.frame_stats(z, per_frame, out=sentinel)
    with pytest.raises(ValueError, match="static plan"):
        cw.transfer_with_plan(z, None, per_frame, content_stats=keep)
    with pytest.raises(ValueError, match="content_stats"):
        cw.transfer_with_plan(z, None, per_frame, by_label=True)
    torch.cuda.synchronize()
    assert untouched()
    transform, redo = per_frame_transforms(cw, binding)
    with pytest.raises(ValueError, match="map_drift"):
        FramePipeline(net, transform, H, W, stats_window=3, stats_by_label=True, map_drift=True)
    with pytest.raises(ValueError, match="stats_window"):
        FramePipeline(net, transform, H, W, stats_by_label=True)
    with pytest.raises(ValueError, match="stats_window"):
        FramePipeline(net, transform, H, W, stats_window=1, stats_by_label=True)
    pipe = FramePipeline(net, transform, H, W, stats_window=3, stats_by_label=True, redo=redo)
    seen = []
    with pytest.raises(ValueError, match="label maps"):                     # no label source
        pipe.run(frames[:2], lambda i, f: seen.append(i))
    with pytest.raises(ValueError, match="warmup"):                         # longer than stats_window - 1 (no seg_window here)
        pipe.run(frames[3:5], lambda i, f: seen.append(i), start_index=3, masks=clip_maps[3:5], warmup=frames[:3],
                 warmup_masks=clip_maps[:3])
    with pytest.raises(ValueError, match="warmup_masks"):                   # one map per warm-up frame
        pipe.run(frames[3:5], lambda i, f: seen.append(i), start_index=3, masks=clip_maps[3:5], warmup=frames[1:3],
                 warmup_masks=clip_maps[:1])
    assert not seen
    plain = FramePipeline(net, transform, H, W)
    with pytest.raises(ValueError, match="warmup_masks"):
        plain.run(frames[:1], lambda i, f: seen.append(i), masks=clip_maps[:1], warmup_masks=[])
    recs = [sentinel, sentinel.clone()]
    tab = per_frame.tables[0]
    with pytest.raises(ValueError, match="plans"):                          # the wrong number of plans
        cw.pool_stats(recs, plans=[tab])
    with pytest.raises(ValueError, match="plan is a contiguous uint8"):     # ... the wrong size
        cw.pool_stats(recs, plans=[tab, tab[:-4]])
    with pytest.raises(ValueError, match="plan is a contiguous uint8"):
        cw.pool_stats(recs, plans=[tab, tab.cpu()])
    with pytest.raises(ValueError, match="plans"):                          # one record, no block
        cw.pool_stats([sentinel[0], sentinel[1]], plans=[tab, tab])
    torch.cuda.synchronize()
    assert untouched()
