"""The optical flow without a GPU: what the numpy statement (tests/flow_ref.py) the device is held to can do on its own - accuracy
on synthetic pairs, fp64 against longdouble, the sign convention against the temporal loss's warp -, the level-count rule, the C
ABI's host-side checks, the parser errors of video_transfer.py --estimate_flow and the two forms of temporal.csv."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import flow_ref as R
import temporal_ref as T
from vstnet_amd import _lib


@functools.lru_cache(maxsize=None)
def case(k):
    """(ref, src, true flow, estimate) of pair k of the table; made once"""
    h, w, levels, amp, shift = R.PAIRS[k]
    ref, src, flow = R.make_pair(h, w, amp, shift)
    return ref, src, flow, R.estimate(ref, src, levels=levels)


@pytest.mark.parametrize("k", range(4))
def test_reference_accuracy(k):
    """A condition on the algorithm: mean interior endpoint error at most 0.1 px and below a tenth of the mean flow magnitude."""
    h, w = R.PAIRS[k][:2]
    _, _, flow, est = case(k)
    mean_epe, max_epe = R.interior_epe(est, flow, h, w)
    mag = float(np.sqrt((flow ** 2).sum(axis=0)).mean())
    print(f"{h}x{w}: mean |flow| {mag:.2f}, interior EPE mean {mean_epe:.4f} max {max_epe:.3f}")
    assert mean_epe <= 0.1 and mean_epe < 0.1 * mag, (mean_epe, mag)


@pytest.mark.parametrize("k", range(4))
def test_fp64_is_enough(k):
    """The fp64 statement and the longdouble one round to the same float32 at every element; float32 arithmetic does not."""
    ref, src, _, est = case(k)
    levels = R.PAIRS[k][2]
    assert np.array_equal(est, R.estimate(ref, src, levels=levels, dtype=np.longdouble))
    low = R.estimate(ref, src, levels=levels, dtype=np.float32)
    assert 0 < np.abs(low - est).max() < 1e-3


def test_sign_convention():
    """Warping src by the estimated flow with the temporal loss's own warp lowers mean |. - ref| on the whole-pixel case."""
    ref, src, flow, est = case(0)
    assert np.allclose(flow[0], 1.0) and np.allclose(flow[1], 0.0)
    _, with_flow = T.l1_u8(src, ref, est)
    _, without = T.l1_u8(src, ref, None)
    assert with_flow.mean() < 0.25 * without.mean(), (with_flow, without)
    _, wrong = T.l1_u8(src, ref, -est)
    assert wrong.mean() > without.mean()


def test_identical_frames_and_the_clamp():
    a = R.to_u8(R.texture(24, 40, 1))
    assert not R.estimate(a, a, levels=2).any()
    b = R.to_u8(R.texture(24, 40, 2))
    d = R.estimate(a, b, levels=1, iters=2, raw=True)
    assert np.abs(d).max() <= 2.0                   # one level: each of the two updates moves a component by at most 1


def test_level_count_rule():
    from vstnet_amd.flow import level_count
    assert R.level_shapes(37, 53, 8) == [(37, 53), (19, 27), (10, 14)]          # 5 x 7 would be the next: shorter edge below 8
    assert R.level_shapes(8, 8, 5) == [(8, 8)] and R.level_shapes(16, 16, 5) == [(16, 16), (8, 8)]
    assert R.level_shapes(15, 400, 5) == [(15, 400), (8, 200)]
    assert len(R.level_shapes(1080, 1920, 5)) == 5 and len(R.level_shapes(1080, 1920, 8)) == 8
    for h, w, lv in ((37, 53, 8), (8, 8, 5), (16, 16, 5), (15, 400, 5), (1080, 1920, 5), (1080, 1920, 8), (96, 128, 1)):
        assert level_count(h, w, lv) == len(R.level_shapes(h, w, lv))


def test_consistency_and_masked_mean_rules():
    h, w = 12, 20
    z = np.zeros((2, h, w), np.float32)
    valid, margin = R.consistency(z, z)
    assert valid.all() and np.allclose(margin, 0.5)
    f = z.copy()
    f[0] = 3.0                                      # forward 3 px right, backward 3 px left: consistent where p - 3 is inside
    valid, _ = R.consistency(f, -f)
    assert valid[:, 3:].all() and not valid[:, :3].any()
    valid, _ = R.consistency(f, f)                  # |6|^2 = 36 > 0.01 * 18 + 0.5
    assert not valid.any()
    a, b = T.make_frame_u8(h, w, 0), T.make_frame_u8(h, w, 1)
    sums, vals = R.l1_masked_u8(a, b, None, np.ones((h, w), np.uint8))
    assert sums[:3] == T.l1_u8(a, b, None)[0] and sums[3] == h * w and vals[3] == 1.0
    assert vals[:3].tobytes() == T.l1_u8(a, b, None)[1].tobytes()
    assert R.l1_masked_u8(a, b, None, np.zeros((h, w), np.uint8))[1].tolist() == [0.0] * 4
    m = np.zeros((h, w), np.uint8)
    m[2, 5] = 1
    sums, vals = R.l1_masked_u8(a, b, None, m)
    assert sums == [abs(int(a[2, 5, c]) - int(b[2, 5, c])) for c in range(3)] + [1] and vals[3] == 1.0 / (h * w)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.vst_version() >= 119
    header = open(os.path.join(_lib.REPO_DIR, "include", "vstnet.h")).read()
    assert "Optical flow (version 119" in header
    for name in ("vst_flow_workspace_bytes", "vst_flow_lk_u8", "vst_flow_consistency", "vst_temporal_l1_masked_u8"):
        assert name in _lib.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    assert (_lib.FLOW_MAX_LEVELS, _lib.FLOW_MAX_ITERS, _lib.FLOW_MAX_RADIUS) == (8, 16, 7)
    for name, v in (("VST_FLOW_MAX_LEVELS", 8), ("VST_FLOW_MAX_ITERS", 16), ("VST_FLOW_MAX_RADIUS", 7)):
        assert f"#define {name} {v}\n" in header
    E_ARG, E_SHAPE = -1, -2
    n = C.c_size_t(0)
    # 4 fp64 planes per level and 7 at the frame's size
    for h, w, levels in ((8, 8, 1), (8, 8, 5), (37, 53, 8), (96, 128, 4), (1080, 1920, 5)):
        px = sum(a * b for a, b in R.level_shapes(h, w, levels))
        assert L.vst_flow_workspace_bytes(h, w, levels, C.byref(n)) == 0 and n.value == 8 * (4 * px + 7 * h * w), (h, w, levels)
    for h, w, levels in ((7, 8, 3), (8, 7, 3), (0, 8, 3), (8193, 8192, 3), (16, 16, 0), (16, 16, 9)):
        assert L.vst_flow_workspace_bytes(h, w, levels, C.byref(n)) == E_SHAPE, (h, w, levels)
    assert L.vst_flow_workspace_bytes(16, 16, 3, None) == E_ARG
    # the launching entry points refuse before they touch anything (non-null addresses that nothing dereferences, far apart)
    a, b, f, g, ws, v = (k << 24 for k in range(1, 7))
    lk = lambda *x: L.vst_flow_lk_u8(*x, None)      # noqa: E731
    assert lk(a, b, 7, 16, 3, 3, 3, 1e-3, f, ws) == E_SHAPE and lk(a, b, 8193, 8192, 3, 3, 3, 1e-3, f, ws) == E_SHAPE
    for levels, iters, radius in ((0, 3, 3), (9, 3, 3), (3, 0, 3), (3, 17, 3), (3, 3, 0), (3, 3, 8)):
        assert lk(a, b, 16, 16, levels, iters, radius, 1e-3, f, ws) == E_SHAPE, (levels, iters, radius)
    for lam in (0.0, -1e-3, float("nan"), float("inf")):
        assert lk(a, b, 16, 16, 3, 3, 3, lam, f, ws) == E_ARG
    for bad in ((None, b, f, ws), (a, None, f, ws), (a, b, None, ws), (a, b, f, None), (a, b, f + 2, ws), (a, b, f, ws + 4),
                (a, b, a, ws), (a, b, b, ws), (a, b, ws, ws), (a, b, ws + 8, ws), (a, b, f, a), (a, b, f, f)):
        assert lk(bad[0], bad[1], 16, 16, 3, 3, 3, 1e-3, bad[2], bad[3]) == E_ARG, bad
    con = lambda *x: L.vst_flow_consistency(*x, None)       # noqa: E731
    assert con(f, g, 7, 16, v) == E_SHAPE and con(f, g, 16, 0, v) == E_SHAPE
    for bad in ((None, g, v), (f, None, v), (f, g, None), (f + 2, g, v), (f, g + 1, v), (f, g, f), (f, g, g + 16)):
        assert con(bad[0], bad[1], 16, 16, bad[2]) == E_ARG, bad
    l1 = lambda *x: L.vst_temporal_l1_masked_u8(*x, None)   # noqa: E731
    assert l1(a, b, None, v, 4, 16, f, None, ws) == E_SHAPE
    for bad in ((None, b, v, f, None, ws), (a, None, v, f, None, ws), (a, b, None, f, None, ws), (a, b, v, None, None, ws),
                (a, b, v, f, None, None), (a, b, v, f + 4, None, ws), (a, b, v, f, None, ws + 4), (a, b, v, f, a, ws),
                (a, b, v, f, b, ws), (a, b, v, f, v, ws)):
        assert l1(bad[0], bad[1], None, bad[2], 16, 16, bad[3], bad[4], bad[5]) == E_ARG, bad
    assert l1(a, b, g + 2, v, 16, 16, f, None, ws) == E_ARG             # the flow off the float grid
    from vstnet_amd import flow
    assert flow.workspace_bytes(96, 128, 4) == 8 * (4 * sum(p * q for p, q in R.level_shapes(96, 128, 4)) + 7 * 96 * 128)
    with pytest.raises(_lib.VstError):
        flow.workspace_bytes(4, 8)


def test_front_end_argument_checks():
    import torch
    from vstnet_amd import flow, temporal
    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        flow.estimate_flow(x, x.clone())            # off the GPU: no fallback
    with pytest.raises(ValueError):
        flow.consistency(torch.zeros((2, 16, 16)), torch.zeros((2, 16, 16)))
    with pytest.raises(ValueError):
        flow.FlowEstimator((16, 16), device="cpu")
    with pytest.raises(ValueError):
        temporal.temporal_loss(x, x.clone(), None, valid=torch.ones((16, 16), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- the script
def test_video_parser_errors(tmp_path, capsys):
    from PIL import Image
    import video_transfer
    img = tmp_path / "still.png"
    Image.fromarray(T.make_frame_u8(64, 96)).save(img)
    clip = tmp_path / "clip"
    clip.mkdir()
    for i in range(3):
        Image.fromarray(T.make_frame_u8(64, 96, i)).save(clip / f"{i:03d}.png")
    flows = tmp_path / "flows"
    flows.mkdir()
    base = ["--style", str(img), "--out_dir", str(tmp_path / "o"), "--synthetic_weights", "--frames_only", "--max_size", "96",
            "--video", str(clip)]
    est = base + ["--temporal", "--estimate_flow"]
    cases = [
        (est + ["--flow_dir", str(flows)], "exactly one source"),
        (base[:-1] + [str(img), "--temporal", "--estimate_flow", "--synthetic_motion", "4"], "exactly one source"),
        (base + ["--temporal", "--flow_dir", str(flows), "--flow_mask"], "--flow_mask"),
        (base + ["--temporal", "--flow_mask"], "exactly one source"),
        (base + ["--estimate_flow"], "belong to --temporal"),
        (base + ["--flow_mask"], "belong to --temporal"),
        (est + ["--flow_levels", "0"], "--flow_levels"),
        (est + ["--flow_levels", "9"], "--flow_levels"),
        (est + ["--flow_iters", "17"], "--flow_iters"),
        (est + ["--flow_radius", "8"], "--flow_radius"),
        (est + ["--flow_lambda", "0"], "--flow_lambda"),
        # the exclusions of --temporal stay, whatever the source
        (est + ["--shard", "0/2"], "--shard"),
        (est + ["--gpus", "2"], "--gpus"),
        (est + ["--upscale", "guided"], "--upscale guided"),
        (est + ["--out_pix_fmt", "yuv420p10le"], "high-bit-depth"),
        (est + ["--stub_stylise"], "--stub_stylise"),
        (base[:6] + ["--max_size", "80", "--video", str(clip), "--temporal", "--estimate_flow"], "stylised at 80x52 and written at 80x64"),
    ]
    for argv, what in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            video_transfer.main(argv)
        assert e.value.code == 2, argv
        assert what in capsys.readouterr().err, (argv, what)
    assert not (tmp_path / "o").exists() or not any(f.endswith(".csv") for _, _, fs in os.walk(tmp_path / "o") for f in fs)


def test_csv_three_and_four_columns(tmp_path):
    from vstnet_amd import flowfiles as FF
    three = {1: (0.1, 0.01), 2: (float("nan"), 0.02)}
    p = FF.write_csv(tmp_path / "a.csv", three, 4)
    assert open(p).read().splitlines() == ["0,,", "1,0.1,0.01", "2,,0.02", "3,,"]
    assert FF.read_csv(p)[1] == (0.1, 0.01) and "valid" not in FF.summary(FF.read_csv(p))
    four = {1: (0.1, 0.01, 0.75), 2: (float("nan"), 0.02, 0.5), 3: (0.3, 0.03, 0.25)}
    p = FF.write_csv(tmp_path / "b.csv", four, 5, valid=True)
    assert open(p).read().splitlines() == ["0,,,", "1,0.1,0.01,0.75", "2,,0.02,0.5", "3,0.3,0.03,0.25", "4,,,"]
    back = FF.read_csv(p)
    assert back[0] == (None, None, None) and back[1] == four[1] and back[2] == (None, 0.02, 0.5)
    assert open(FF.write_csv(tmp_path / "c.csv", back, valid=True), "rb").read() == open(p, "rb").read()
    line = FF.summary(back)
    assert "2 frame pairs" in line and line.endswith("mean valid share 0.5000")
    open(tmp_path / "bad.csv", "w").write("0,1.0,2.0,3.0,4.0\n")
    with pytest.raises(ValueError, match="bad.csv line 1"):
        FF.read_csv(tmp_path / "bad.csv")
