"""The statistics window (--stats_window, DESIGN.md section 5 "Statistics window") on the GPU: vst_cwct_stats_pool against a
long-double truth over the whole case table, the window through the real statistics kernels against fp64 statistics of the
union of the frames' pixels, FramePipeline(stats_window=...) against a serial restatement (also on the static-mask route, with
warm-up frames and in artistic mode), video_transfer.py with shards, the drift of the affine map, the scene cut and the errors.

Bounds.  Kernel: device <= 4 x max(e64, 2^-53) under the statistics metrics with the pooled C, e64 = the fp64 restatement against
the same truth (tests/stats_window_ref.py); `used` equal; records under the copy rule equal as bits.  Through the statistics
kernels: FACTOR['stats'] x max(e32, U) of tests/cwct_ops_ref.py, e32 = stats32 per frame pooled by the fp64 restatement.
Pipelines and shards: byte equality.  Drift: >= 0.1 per step at W = 1 (the CPU oracle gives 0.63 and 1.13), <= 1e-3 (the
project's north-star budget) from the third frame on at W = 2: the two windows hold the same two records in opposite order, their
pooled records differ at the 1e-16 level, and the fp32 factor's outputs by its own conditioning noise (about 2e-4 at cond 3e3).
The figures are printed before they are asserted (-s)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import cwct_ops_ref as O
import stats_window_ref as R
from vstnet_amd.synth import synthetic_mask, synthetic_scene_u8, synthetic_state_dict

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 64, 96
N_FRAMES = 7
NAN64 = float("nan")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def cw():
    from models.cWCT import cWCT
    return cWCT()


def make_net(mode):
    from models.RevResNet import RevResNet
    hd, sp = (16, 2) if mode == "photo" else (64, 1)
    n = RevResNet(hidden_dim=hd, sp_steps=sp)
    n.load_state_dict(synthetic_state_dict(1234, hd, sp))
    return n.to("cuda").eval()


@pytest.fixture(scope="module")
def net():
    return make_net("photo")


@pytest.fixture(scope="module")
def frames():
    return [synthetic_scene_u8(H, W, 60 + i) for i in range(N_FRAMES)]


def style_code(net, seed=77, hw=(48, 64)):
    with torch.no_grad():
        return net.forward_u8(torch.from_numpy(synthetic_scene_u8(hw[0], hw[1], seed)).cuda()[None])


# ------------------------------------------------------------------------------------------------------ 1. the kernel against truth
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


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_pool_kernel_against_truth(cw, case):
    N, n_rec = case[0], case[1]
    records, weights, cut = R.case_input(case)
    truth, used = R.pool_ref(records, weights, cut, np.longdouble)
    r64, _ = R.pool_ref(records, weights, cut)
    ins = [Margins(r.shape, NAN64) for r in records]
    for m, r in zip(ins, records):
        m.view.copy_(torch.from_numpy(r))
    out = Margins(records[0].shape, O.SENTINEL_F64)
    d_used = torch.full((n_rec + 2,), -7, dtype=torch.int32, device="cuda")
    got_t = cw.pool_stats([m.view for m in ins], weights=weights, cut=cut, out=out.view, used=d_used[1:1 + n_rec])
    assert got_t.data_ptr() == out.view.data_ptr()
    got, got_used = out.view.cpu().numpy(), d_used.cpu().numpy()
    ratio, (gc, gm, ec, em) = R.pool_ratio(got, r64, truth, used, N)
    print(f"pool {R.case_id(case)}: e64 cov {ec:.3g} mean {em:.3g}, device cov {gc:.3g} mean {gm:.3g} = {ratio:.2f} x, bound {R.FACTOR}")
    assert np.array_equal(got_used[1:1 + n_rec], used) and got_used[0] == -7 == got_used[-1]
    for r in range(n_rec):
        if used[r] <= 1:                                   # the copy rule: the bits of the age-0 record, NaNs and all
            assert bits(got[r]).tobytes() == bits(records[0][r]).tobytes(), r
    assert out.margins_untouched() and all(m.margins_untouched() for m in ins)
    for m, r in zip(ins, records):                         # (the inputs are only read)
        assert bits(m.view.cpu().numpy()).tobytes() == bits(r).tobytes()
    assert ratio <= R.FACTOR, (R.case_id(case), ratio)


# ------------------------------------------------------------------------------------- 2. through the real statistics kernels
def frame_inputs(N, shape, frames=3):
    return [O.stats_input(N, int(np.prod(shape)), "scales", seed=11 + f).reshape((N,) + tuple(shape)) for f in range(frames)]


def pooled_bound_check(name, got, per_frame32, xs_cols, N, skip):
    """got: the device's pooled record; per_frame32: the frames' restated fp32 records (newest first, like got's inputs);
    xs_cols: the frames' columns [N, L_f] -> asserts the bound against stats64 of their union"""
    want = O.stats64(np.concatenate(xs_cols, axis=1))
    r32, used = R.pool_ref(per_frame32, np.ones(len(per_frame32)), 0.0)
    assert used[0] == len(per_frame32) and got[0] == want[0]
    r, (gc, gm, ec, em) = O.stats_ratio(got, r32[0], want, N, skip=skip)
    print(f"{name}: e32 cov {ec / O.U:.3g} u mean {em / O.U:.3g} u, device cov {gc / O.U:.3g} u mean {gm / O.U:.3g} u = {r:.2f} x, "
          f"bound {O.FACTOR['stats']}")
    assert r <= O.FACTOR["stats"], (name, r)


@pytest.mark.parametrize("sp,Hc,Wc", [(2, 24, 40), (1, 24, 40)])
def test_window_through_the_packed_statistics(cw, sp, Hc, Wc):
    from vstnet_amd.code import from_dense
    N, shape = (32, (Hc, Wc)) if sp == 2 else (128, (Hc // 2, Wc // 2))
    zs = frame_inputs(N, shape)
    L, per = O.code_groups(Hc, Wc, sp)
    recs, r32, cols = [], [], []
    for z in zs:
        code = from_dense(torch.from_numpy(z)[None].cuda())
        recs.append(cw.frame_stats(code))
        assert cw.last_route == "packed_rows"
        rows = code.packed.cpu().numpy().reshape(-1, N)      # the code's own rows: the order of the channels in a row is its own
        y, x = O.row_pixels(Hc, Wc, sp)
        assert (np.sort(rows, axis=1) == np.sort(z[:, y, x].T, axis=1)).all(), "row order"
        cols.append(np.ascontiguousarray(rows.T))
        r32.append(O.stats32(cols[-1], groups=(-(-L // per), per, "code")))
    const = int(np.nonzero((rows == O.CONST_VAL).all(0))[0][0])
    got = cw.pool_stats(recs[::-1]).cpu().numpy()
    pooled_bound_check(f"window on packed rows sp={sp} {Hc}x{Wc}", got, r32[::-1], cols, N, (const,))


@pytest.mark.parametrize("N,shape", [(16, (12, 43)), (8, (7, 247))])
def test_window_through_the_dense_statistics(cw, N, shape):
    zs = frame_inputs(N, shape)
    recs = [cw.frame_stats(torch.from_numpy(z)[None].cuda()) for z in zs]
    assert cw.last_route == ("dense" if N == 16 else "any_width_dense")
    cols = [z.reshape(N, -1) for z in zs]
    got = cw.pool_stats(recs[::-1]).cpu().numpy()
    pooled_bound_check(f"window on dense codes N={N} L={cols[0].shape[1]}", got, [O.stats32(c) for c in cols][::-1], cols, N,
                       (O.CONST_CH,))


# ------------------------------------------------------------------------------------------------------- 3. static-mask records
def test_window_of_static_mask_records(cw):
    """Nine slots: more than the packed masked route takes, so the route of this packed code is the single-pass one on the
    materialised code (vst_cwct_stats_labels), which is what frame_stats must then run."""
    from vstnet_amd.code import from_dense
    Hc, Wc, n = 72, 104, 9
    mask = O.code_label_mask(Hc, Wc, n)
    lut, labels, over = O.plan_ref(mask, mask)
    assert len(labels) == n and not over
    mid = mask.copy()
    mid[mid == labels[4]] = labels[5]                      # the middle frame lacks one label: that slot's record has n = 0
    plan = cw.learn_slots(cw.plan_masks(mask[None], mask[None], (1, 32, Hc, Wc), (1, 32, Hc, Wc), "cuda"))
    assert plan.max_slots == n
    plan_mid = copy.copy(plan)                             # the same table (slots), another map
    plan_mid.cm = [torch.from_numpy(mid.reshape(-1)).cuda()]
    zs = frame_inputs(32, (Hc, Wc))
    masks = [mask, mid, mask]
    recs, r32, cols = [], [], []
    for z, m, pl in zip(zs, masks, (plan, plan_mid, plan)):
        out = torch.full((O.MAX_SLOTS, O.rec_len(32)), O.SENTINEL_F64, dtype=torch.float64, device="cuda")
        assert cw.frame_stats(from_dense(torch.from_numpy(z)[None].cuda()), pl, out=out) is out
        assert cw.last_route == "masked_single_pass"
        recs.append(out)
        cols.append(np.ascontiguousarray(z.reshape(32, -1)))
        r32.append(O.stats_labels32(cols[-1], m.reshape(-1), lut, n, n))
    assert float(recs[1][4, 0]) == 0.0
    used = torch.zeros(O.MAX_SLOTS, dtype=torch.int32, device="cuda")
    got = cw.pool_stats(recs[::-1], used=used).cpu().numpy()
    want = O.stats_labels64(np.concatenate(cols, axis=1), np.concatenate([m.reshape(-1) for m in masks]), lut, n)
    p32, u32 = R.pool_ref([r[:n] for r in r32[::-1]], np.ones(3), 0.0)
    assert np.array_equal(used.cpu().numpy()[:n], u32) and u32[4] == 2 and set(np.delete(u32, 4)) == {3}
    worst = 0.0
    for s in range(n):
        assert got[s, 0] == want[s, 0], ("count", s)
        worst = max(worst, O.stats_ratio(got[s], p32[s], want[s], 32, skip=(O.CONST_CH,))[0])
    print(f"window of per-slot records {Hc}x{Wc} slots={n}: device {worst:.2f} x max(e32, floor), bound {O.FACTOR['stats']}")
    assert worst <= O.FACTOR["stats"]


# ------------------------------------------------------------------------------------------- 4.-8. the pipeline against serial
def static_plan(cw, z_s, hw=(H, W), sp=2):
    cseg, sseg = synthetic_mask(hw[0], hw[1], labels=5, seed=3), synthetic_mask(z_s.shape[2], z_s.shape[3], labels=5, seed=4)
    plan = cw.plan_masks(cseg[None], sseg[None], (1, 32, hw[0], hw[1]), tuple(z_s.shape), "cuda")
    return cw.bind_style(cw.learn_slots(plan), z_s)


def transfer(cw, s_stats, plan):
    if plan is not None:
        return lambda z, **kw: cw.transfer_with_plan(z, None, plan, **kw)
    return lambda z, **kw: cw.transfer_with_stats(z, s_stats, **kw)


def run_pipeline(net, cw, clip, s_stats=None, plan=None, start=0, warmup=(), depth=3, streams=2, **kw):
    """{frame index: stylised uint8 frame} of FramePipeline over `clip`"""
    from vstnet_amd.pipeline import FramePipeline
    seen, tr = {}, transfer(cw, s_stats, plan)
    if kw.get("stats_window", 1) > 1 or "frame_stats" in kw:
        kw.setdefault("frame_stats", lambda z, out=None: cw.frame_stats(z, plan, out=out))
    pipe = FramePipeline(net, lambda z, i, **k: tr(z, **k), clip[0].shape[0], clip[0].shape[1], depth=depth,
                         compute_streams=streams, **kw)
    n = pipe.run(clip, lambda i, f: seen.__setitem__(i, f.copy()), start_index=start, warmup=warmup)
    assert n == len(clip) and sorted(seen) == list(range(start, start + n))
    return pipe, seen


def run_serial(net, cw, clip, window, decay=1.0, cut=0.0, s_stats=None, plan=None):
    """One stream, the same library calls in frame order"""
    tr, ring, outs = transfer(cw, s_stats, plan), [], []
    with torch.no_grad():
        for f in clip:
            z = net.forward_u8(torch.from_numpy(f).cuda()[None])
            ring = ([cw.frame_stats(z, plan)] + ring)[:window]
            pooled = cw.pool_stats(ring, decay=decay, cut=cut)
            outs.append(net.inverse_u8(tr(z, content_stats=lambda rec, b: pooled))[0].cpu().numpy())
    return outs


@pytest.fixture(scope="module")
def photo(net, cw, frames):
    """the unmasked route's style side, the W = 3, D = 0.5 serial frames and the full pipeline run, computed once"""
    s_stats = cw.style_stats(style_code(net))
    want = run_serial(net, cw, frames, 3, 0.5, s_stats=s_stats)
    pipe, seen = run_pipeline(net, cw, frames, s_stats=s_stats, stats_window=3, stats_decay=0.5)
    return s_stats, want, pipe, seen


def test_pipeline_equals_serial(net, cw, frames, photo):
    s_stats, want, pipe, seen = photo
    assert tuple(pipe.stat_ring.shape) == (3 + 3, O.rec_len(32)) and pipe.stat_window.slots == 6
    for i in range(N_FRAMES):
        assert np.array_equal(seen[i], want[i]), i
    assert [pipe.window_used[i] for i in range(N_FRAMES)] == [(1, 1), (2, 2)] + [(3, 3)] * (N_FRAMES - 2)
    _, plain = run_pipeline(net, cw, frames, s_stats=s_stats)
    assert np.array_equal(plain[0], want[0]) and not np.array_equal(plain[2], want[2])      # (the window does change the frames)


def test_pipeline_equals_serial_artistic(cw):
    art = make_net("art")
    clip = [synthetic_scene_u8(H, W, 60 + i) for i in range(4)]
    s_stats = cw.style_stats(style_code(art))
    want = run_serial(art, cw, clip, 2, s_stats=s_stats)
    pipe, seen = run_pipeline(art, cw, clip, s_stats=s_stats, stats_window=2)
    assert tuple(pipe.stat_ring.shape) == (2 + 3, O.rec_len(128))
    for i in range(4):
        assert np.array_equal(seen[i], want[i]), i


def test_pipeline_equals_serial_static_mask(net, cw, frames):
    plan = static_plan(cw, style_code(net))
    assert plan.max_slots == 5
    want = run_serial(net, cw, frames, 3, 0.5, plan=plan)
    pipe, seen = run_pipeline(net, cw, frames, plan=plan, stats_window=3, stats_decay=0.5)
    assert cw.last_route == "masked_packed_rows" and tuple(pipe.stat_ring.shape) == (6, 32, O.rec_len(32))
    for i in range(N_FRAMES):
        assert np.array_equal(seen[i], want[i]), i
    assert not np.array_equal(run_serial(net, cw, frames[:3], 1, plan=plan)[2], want[2])


def test_window_1_is_todays_route(net, cw, frames, photo):
    s_stats = photo[0]
    clip = frames[:4]
    pipe, one = run_pipeline(net, cw, clip, s_stats=s_stats, stats_window=1)
    assert getattr(pipe, "stat_ring", None) is None and pipe.stat_window is None and pipe.h_aff is None
    _, plain = run_pipeline(net, cw, clip, s_stats=s_stats)
    from vstnet_amd.pipeline import FramePipeline
    seen = {}
    same = FramePipeline(net, lambda z, i: cw.transfer_with_stats(z, s_stats, content_stats=lambda rec, b: rec), H, W, depth=3)
    same.run(clip, lambda i, f: seen.__setitem__(i, f.copy()))
    for i in range(4):
        assert np.array_equal(one[i], plain[i]) and np.array_equal(seen[i], plain[i]), i


def test_warmup_frames_give_a_shard_the_full_runs_frames(net, cw, frames, photo):
    s_stats, want, _, _ = photo
    _, seen = run_pipeline(net, cw, frames[3:], s_stats=s_stats, start=3, warmup=frames[1:3], stats_window=3, stats_decay=0.5)
    for i in range(3, N_FRAMES):
        assert np.array_equal(seen[i], want[i]), i
    _, cold = run_pipeline(net, cw, frames[3:], s_stats=s_stats, start=3, stats_window=3, stats_decay=0.5)
    assert not np.array_equal(cold[3], want[3])              # the window started over
    for i in range(5, N_FRAMES):                             # ... and has filled by frame 5
        assert np.array_equal(cold[i], want[i]), i


def test_video_transfer_stats_window_and_two_shards(tmp_path, frames):
    import video_transfer
    fd = tmp_path / "clip"
    fd.mkdir()
    for i, f in enumerate(frames):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
    Image.fromarray(synthetic_scene_u8(72, 104, 50)).save(tmp_path / "s.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only", "--stats_window", "3",
            "--stats_decay", "0.5"]
    one = video_transfer.main(base + ["--out_dir", str(tmp_path / "o1")])
    names = ["%05d.png" % i for i in range(N_FRAMES)]
    assert sorted(os.listdir(one)) == names
    plain = video_transfer.main(base[:-4] + ["--out_dir", str(tmp_path / "o0")])
    differ = [not np.array_equal(np.asarray(Image.open(os.path.join(one, n))), np.asarray(Image.open(os.path.join(plain, n))))
              for n in names]
    assert not differ[0] and all(differ[1:])                 # the flag reaches the frames
    # the two shards one after the other, each in a fresh process with its own time limit
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    for shard in ("0/2", "1/2"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py")] + base
                           + ["--out_dir", str(tmp_path / "o2"), "--shard", shard], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (shard, r.stderr[-3000:])
    two = os.path.join(str(tmp_path / "o2"), os.path.basename(one))
    assert sorted(os.listdir(two)) == names
    for n in names:
        assert np.array_equal(np.asarray(Image.open(os.path.join(one, n))), np.asarray(Image.open(os.path.join(two, n)))), n


@pytest.fixture(scope="module")
def scenes():
    return R.scenes_u8(48, 64)


def test_map_drift(net, cw, scenes):
    A, B = scenes
    clip = [A, B, A, B, A, B]
    s_stats = cw.style_stats(style_code(net))
    p1, _ = run_pipeline(net, cw, clip, s_stats=s_stats, map_drift=True)
    p2, _ = run_pipeline(net, cw, clip, s_stats=s_stats, stats_window=2, map_drift=True)
    d1, d2 = [p1.drifts[i] for i in range(1, 6)], [p2.drifts[i] for i in range(1, 6)]
    print("drift of the affine map, W = 1:", " ".join(f"{d:.3g}" for d in d1), "| W = 2:", " ".join(f"{d:.3g}" for d in d2))
    assert sorted(p1.drifts) == sorted(p2.drifts) == [1, 2, 3, 4, 5]
    assert p1.mean_drift == pytest.approx(np.mean(d1), rel=1e-12)
    assert min(d1) >= 0.1
    assert max(d2[1:]) <= 1e-3


def test_scene_cut(net, cw, scenes, tmp_path):
    import video_transfer
    A, B = scenes
    clip = [A, R.noisy_u8(A, 1), R.noisy_u8(A, 2), B, R.noisy_u8(B, 3), R.noisy_u8(B, 4)]
    s_stats = cw.style_stats(style_code(net))
    pipe, seen = run_pipeline(net, cw, clip, s_stats=s_stats, stats_window=3, stats_cut=R.CUT_T)
    used = [pipe.window_used[i][0] for i in range(6)]
    print("frames pooled per frame:", used)
    assert used == [1, 2, 3, 1, 2, 3] and pipe.stats_cuts == 1
    _, plain = run_pipeline(net, cw, clip, s_stats=s_stats)
    assert np.array_equal(seen[3], plain[3]) and not np.array_equal(seen[2], plain[2])
    _, uncut = run_pipeline(net, cw, clip, s_stats=s_stats, stats_window=3)
    assert not np.array_equal(uncut[3], plain[3])            # (without the cut, scene A reaches scene B's first frame)
    fd = tmp_path / "clip"
    fd.mkdir()
    for i, f in enumerate(clip):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
    Image.fromarray(synthetic_scene_u8(48, 64, 77)).save(tmp_path / "s.png")
    out = video_transfer.main(["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only",
                               "--stats_window", "3", "--stats_cut", str(R.CUT_T), "--map_drift", "--out_dir", str(tmp_path / "o")])
    assert video_transfer.LAST_RUN["stats_cuts"] == 1 and video_transfer.LAST_RUN["map_drift"] > 0
    for i in range(6):
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "%05d.png" % i))), seen[i]), i


# ------------------------------------------------------------------------------------------------------------------- 9. errors
def test_pool_errors_launch_nothing():
    from vstnet_amd import _lib
    import ctypes as C
    L, vp = _lib.lib(), C.c_void_p
    N, n_rec = 32, 2
    count = n_rec * O.rec_len(N)
    recs = torch.full((2 * count + 2,), 3.0, dtype=torch.float64, device="cuda")
    out = torch.full((2 * count,), O.SENTINEL_F64, dtype=torch.float64, device="cuda")      # (room on both sides of the record)
    used = torch.full((n_rec,), -7, dtype=torch.int32, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    o = out.data_ptr() + 8 * (count // 2)
    for name, status, a in R.pool_error_cases(recs.data_ptr(), o, N, n_rec):
        a = a[:7] + (vp(used.data_ptr()),)
        assert L.vst_cwct_stats_pool(*a, st) == status, name
    with pytest.raises(_lib.VstError, match="-2"):
        _lib.check(L.vst_cwct_stats_pool((vp * 1)(recs.data_ptr()), (C.c_double * 1)(1.0), 9, n_rec, N, 0.0, vp(o), None, st),
                   "vst_cwct_stats_pool")
    torch.cuda.synchronize()
    assert bits(out.cpu().numpy()).tobytes() == bits(np.full(2 * count, O.SENTINEL_F64)).tobytes()
    assert used.tolist() == [-7, -7] and float(recs.min()) == 3.0 == float(recs.max())
    # and the same call, valid, runs: two ages of records {3, 3, ...}: n = 3 each, equal means, C = 3
    ptrs, w = (vp * 2)(recs.data_ptr(), recs.data_ptr() + 8 * count), (C.c_double * 2)(1.0, 0.5)
    assert L.vst_cwct_stats_pool(ptrs, w, 2, n_rec, N, 0.0, vp(o), vp(used.data_ptr()), st) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert used.tolist() == [2, 2] and got[count // 2] == 4.5 and np.all(got[count // 2 + 1:count // 2 + 1 + N] == 3.0)
    assert np.all(got[:count // 2] == O.SENTINEL_F64) and np.all(got[count // 2 + count:] == O.SENTINEL_F64)


# ------------------------------------------------------------------------------------------------------------------ 10. guards
def test_guards(net, cw, frames):
    from vstnet_amd.pipeline import FramePipeline
    z_s = style_code(net)
    s_stats = cw.style_stats(z_s)
    keep = lambda rec, b: rec      # noqa: E731
    with torch.no_grad():
        z = net.forward_u8(torch.from_numpy(frames[0]).cuda()[None])
    sseg = synthetic_mask(z_s.shape[2], z_s.shape[3], labels=5, seed=4)
    binding = cw.bind_style_labels(z_s, sseg)
    per_frame = cw.plan_frame(torch.from_numpy(synthetic_mask(H, W, labels=5, seed=3)).cuda(), binding)
    torch.cuda.synchronize()
    sentinel = torch.full((32, O.rec_len(32)), O.SENTINEL_F64, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="static plan"):
        cw.transfer_with_plan(z, None, per_frame, content_stats=keep)
    with pytest.raises(ValueError, match="static plan"):
        cw.frame_stats(z, per_frame, out=sentinel)
    assert bits(sentinel.cpu().numpy()).tobytes() == bits(np.full((32, O.rec_len(32)), O.SENTINEL_F64)).tobytes()
    fs = lambda zc, out=None: cw.frame_stats(zc, out=out)      # noqa: E731
    tr = lambda zc, i, *a, **k: cw.transfer_with_stats(zc, s_stats, **k)      # noqa: E731
    with pytest.raises(ValueError, match="segmenter"):
        FramePipeline(net, tr, H, W, segmenter=object(), stats_window=3, frame_stats=fs)
    with pytest.raises(ValueError, match="frame_stats"):
        FramePipeline(net, tr, H, W, stats_window=3)
    for bad in (dict(stats_window=0), dict(stats_window=9), dict(stats_window=2, stats_decay=0.0), dict(stats_window=2, stats_cut=-1.0)):
        with pytest.raises(ValueError, match="stats_"):
            FramePipeline(net, tr, H, W, frame_stats=fs, **bad)
    pipe = FramePipeline(net, tr, H, W, stats_window=3, frame_stats=fs)
    seen = []
    with pytest.raises(ValueError, match="label maps"):
        pipe.run(frames[:2], lambda i, f: seen.append(i), masks=[synthetic_mask(H, W, labels=5, seed=3)] * 2)
    assert not seen and pipe.stat_ring is None               # nothing was submitted
    with pytest.raises(ValueError, match="1..8"):
        cw.pool_stats([sentinel[0]] * 9)
    with pytest.raises(ValueError, match="one shape"):
        cw.pool_stats([sentinel[0], sentinel])
    with pytest.raises(ValueError, match="decay"):
        cw.pool_stats([sentinel[0]], decay=1.5)
