"""The temporal loss without a GPU: the yardstick (tests/temporal_ref.py) against the reference's own warp and forward
(tests/golden/temporal.npz, written by tests/make_temporal_golden.py), the flow and csv files (vstnet_amd/flowfiles.py), the C
ABI's host-side checks, every parser error of video_transfer.py --temporal, and the reference's import path without OpenCV."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import temporal_ref as R
from vstnet_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_SIZES = R.SIZES[:3]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "temporal.npz"))


@pytest.mark.parametrize("h,w", GOLDEN_SIZES)
@pytest.mark.parametrize("kind", R.FLOW_KINDS)
def test_ref_equals_the_reference(gold, h, w, kind):
    """The fp32 restatement reads, at every pixel, the pixel torch's CPU grid_sample read on the reference's grid; the loss of
    forward agrees to the reference's own float32 arithmetic (|a - b| and its mean in float32: 2^-24 per term and per partial sum,
    bounded by 2e-6 relative at these sizes)."""
    key = f"{h}x{w}_{kind}"
    flow = gold[key + "_flow"]
    assert np.array_equal(flow, R.make_flow(h, w, kind)), "the golden file was made from other inputs than temporal_ref's"
    sy, sx = R.source_index(flow, h, w)
    assert np.array_equal(sy * w + sx, gold[key + "_src"])
    if kind == "zero":
        assert np.array_equal(sy * w + sx, np.arange(h * w).reshape(h, w))
    first, second = gold[f"{h}x{w}_first"], gold[f"{h}x{w}_second"]
    assert np.array_equal(first, R.make_frame_f32(h, w, 0)) and np.array_equal(second, R.make_frame_f32(h, w, 1))
    mine = float(R.l1_f32(first, second, flow).mean())
    assert abs(mine - float(gold[key + "_loss"])) <= 2e-6 * mine
    # the share of pixels a warp test may exempt, on the golden cases too (the GPU test asserts it on every case it runs)
    share = float(R.near_tie(flow, h, w).mean())
    assert share == float(gold[key + "_near_tie"]) and share <= 1e-3, (key, share)
    if kind in ("integer", "zero"):
        assert share == 0.0
    assert float(gold["real_scale"]) == 3.0


def test_ref_noise_and_l1_rules():
    h, w = 5, 7
    x = R.make_frame_u8(h, w)
    n = np.zeros((3, h, w), np.float32)
    n[0], n[1], n[2] = 2.0, -2.0, 0.5 / 255.0              # saturates up, saturates down, a tie: 0.5 rounds to even
    out = R.warp_u8(x, None, n)
    assert (out[..., 0] == 255).all() and (out[..., 1] == 0).all()
    assert np.array_equal(out[..., 2], np.rint(x[..., 2].astype(np.float32) + np.float32(0.5)).clip(0, 255).astype(np.uint8))
    sums, vals = R.l1_u8(x, x, None)
    assert sums == [0, 0, 0] and (vals == 0.0).all()
    y = x.copy()
    y[0, 0, 1] ^= 0xFF
    sums, vals = R.l1_u8(x, y, None)
    assert sums[0] == 0 and sums[1] == abs(int(x[0, 0, 1]) - int(y[0, 0, 1])) and vals[1] == sums[1] / (255.0 * h * w)
    a, b = R.make_frame_f32(h, w, 0), R.make_frame_f32(h, w, 1)
    want = np.abs(a.astype(np.float64) - b.astype(np.float64)).reshape(3, -1).mean(axis=1)
    assert np.abs(R.l1_f32(a, b, None) - want).max() <= 1e-15


def test_ref_fake_flow_properties():
    """A constant grid gives that constant plus the shifts (both steps' weights add up to one); ksize 1 is the upsample alone;
    and the field is smooth: neighbouring pixels differ by far less than the grid's deviation."""
    g = np.full((3, 4, 2), 2.5)
    f = R.fake_flow(g, (3, -4), 30, 44, 9)
    assert np.abs(f[0] - 5.5).max() < 1e-13 and np.abs(f[1] + 1.5).max() < 1e-13
    grid, shifts = R.flow_draws(37, 53, 10)
    up = R.fake_flow(grid, (0, 0), 37, 53, 1)
    assert abs(up[0, 0, 0] - grid[0, 0, 0]) < 1e-13 and abs(up[1, -1, -1] - grid[-1, -1, 1]) < 1e-13      # edges replicated
    f = R.fake_flow(grid, shifts, 37, 53, 7)
    assert np.abs(np.diff(f, axis=2)).max() < 8.0 / 2 and np.abs(np.diff(f, axis=1)).max() < 8.0 / 2
    # the box filter against a direct double loop on one pixel near a corner (reflect-101: the edge pixel is not repeated)
    u = up + np.array(shifts, np.float64)[:, None, None]
    y, x, k = 1, 51, 7
    acc = 0.0
    for dy in range(k):
        for dx in range(k):
            yy, xx = abs(y - k // 2 + dy), x - k // 2 + dx
            xx = 2 * 52 - xx if xx > 52 else xx
            acc += u[0, yy, xx]
    assert abs(acc / 49 - f[0, y, x]) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- the files
def test_flo_round_trip_and_errors(tmp_path):
    from vstnet_amd import flowfiles as FF
    flow = R.make_flow(12, 20, "real")
    p = FF.write_flo(tmp_path / "a.flo", flow)
    raw = open(p, "rb").read()
    assert len(raw) == 12 + 8 * 12 * 20 and raw[:4] == np.float32(202021.25).tobytes() and raw[4:12] == np.array([20, 12], "<i4").tobytes()
    assert raw[12:20] == np.array([flow[0, 0, 0], flow[1, 0, 0]], "<f4").tobytes()            # interleaved (u, v)
    back = FF.read_flo(p)
    assert back.dtype == np.float32 and np.array_equal(back, flow)
    assert np.array_equal(FF.read_flow(str(p), (12, 20), negate=True), -flow)
    np.save(tmp_path / "b.npy", flow.astype(np.float64))
    got = FF.read_flow(str(tmp_path / "b.npy"), (12, 20))
    assert got.dtype == np.float32 and np.array_equal(got, flow)
    open(tmp_path / "bad.flo", "wb").write(b"PIEH" + raw[4:-8])
    with pytest.raises(ValueError, match="bad.flo"):
        FF.read_flo(tmp_path / "bad.flo")
    open(tmp_path / "short.flo", "wb").write(raw[:-8])
    with pytest.raises(ValueError, match=r"short.flo.*20x12"):
        FF.read_flo(tmp_path / "short.flo")
    open(tmp_path / "tiny.flo", "wb").write(raw[:7])
    with pytest.raises(ValueError, match="tiny.flo"):
        FF.read_flo(tmp_path / "tiny.flo")
    with pytest.raises(ValueError, match=r"a.flo.*20x12.*24x12"):
        FF.read_flow(str(p), (12, 24))
    np.save(tmp_path / "c.npy", flow[0])
    with pytest.raises(ValueError, match="c.npy"):
        FF.read_flow(str(tmp_path / "c.npy"))
    with pytest.raises(ValueError, match="x.txt"):
        FF.read_flow(str(tmp_path / "x.txt"))
    d = tmp_path / "flows"
    d.mkdir()
    for j in (1, 0):
        FF.write_flo(d / f"{j:03d}.flo", flow)
    np.save(d / "002.npy", flow)
    assert [os.path.basename(f) for f in FF.list_flows(str(d), 4)] == ["000.flo", "001.flo", "002.npy"]
    with pytest.raises(ValueError, match="3 flow files.*5 frames has 4"):
        FF.list_flows(str(d), 5)


def test_csv_round_trip_and_summary(tmp_path):
    from vstnet_amd import flowfiles as FF
    rows = {1: (0.1 + 1e-9 / 3, 0.01), 2: (float("nan"), 0.02), 3: (0.3, 0.015)}
    p = FF.write_csv(tmp_path / FF.CSV_NAME, rows, 5)
    lines = open(p).read().splitlines()
    assert lines[0] == "0,," and lines[1] == "1,%r,%r" % rows[1] and lines[2] == "2,,0.02" and lines[4] == "4,,"
    back = FF.read_csv(p)
    assert back[0] == (None, None) and back[1] == rows[1] and back[2] == (None, 0.02) and back[3] == rows[3]
    assert open(FF.write_csv(tmp_path / "again.csv", back), "rb").read() == open(p, "rb").read()
    line = FF.summary(back)
    assert "2 frame pairs" in line and "(frame 3)" in line and "amplification 16.000" in line
    assert "%.6e" % ((rows[1][0] + 0.3) / 2) in line and "%.6e" % 0.0125 in line
    assert FF.summary({}) == "temporal: no frame pairs" and FF.summary({0: (None, None)}) == "temporal: no frame pairs"
    open(tmp_path / "bad.csv", "w").write("0,1.0\n")
    with pytest.raises(ValueError, match="bad.csv line 1"):
        FF.read_csv(tmp_path / "bad.csv")


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.vst_version() >= 118
    names = ("vst_warp_u8", "vst_warp_f32", "vst_temporal_workspace_bytes", "vst_temporal_l1_u8", "vst_temporal_l1_f32",
             "vst_fake_flow_workspace_bytes", "vst_fake_flow")
    header = open(os.path.join(_lib.REPO_DIR, "include", "vstnet.h")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    E_ARG, E_SHAPE = -1, -2
    n = C.c_size_t(0)
    # 24 bytes per workgroup of 2048 pixels
    for (h, w), blocks in (((8, 8), 1), ((37, 53), 1), ((128, 260), 17), ((1080, 1920), 1013), ((1, 2049), 2)):
        assert L.vst_temporal_workspace_bytes(h, w, C.byref(n)) == 0 and n.value == 24 * blocks, (h, w, n.value)
    for h, w in ((0, 8), (8, 0), (-1, 8), (8193, 8192)):
        assert L.vst_temporal_workspace_bytes(h, w, C.byref(n)) == E_SHAPE
    assert L.vst_temporal_workspace_bytes(8, 8, None) == E_ARG
    assert L.vst_fake_flow_workspace_bytes(200, 300, 2, 3, 100, C.byref(n)) == 0 and n.value == 8 * (300 * 3 + 200 * 2 + 2 * 2 * 300)
    # the launching entry points refuse before they touch anything (p, q: non-null addresses nothing dereferences)
    p, q = 4096, 8192
    bad_flow = ((16, 20, 0, 5, 6), (16, 20, 4, 0, 6), (16, 20, 4, 5, 17), (16, 20, 4, 5, 0), (20, 16, 4, 5, 17), (16, 20, 1025, 5, 6),
                (0, 20, 4, 5, 6), (8193, 8192, 4, 5, 6))
    for h, w, gh, gw, k in bad_flow:
        assert L.vst_fake_flow_workspace_bytes(h, w, gh, gw, k, C.byref(n)) == E_SHAPE, (h, w, gh, gw, k)
        assert L.vst_fake_flow(p, gh, gw, 0.0, 0.0, k, p, h, w, p, None) == E_SHAPE, (h, w, gh, gw, k)
    assert L.vst_fake_flow(None, 4, 5, 0.0, 0.0, 6, p, 16, 20, p, None) == E_ARG
    assert L.vst_fake_flow(p, 4, 5, float("nan"), 0.0, 6, p, 16, 20, p, None) == E_ARG
    assert L.vst_fake_flow(p + 4, 4, 5, 0.0, 0.0, 6, p, 16, 20, p, None) == E_ARG
    for fn in (L.vst_warp_u8, L.vst_warp_f32):
        assert fn(p, p, None, q, 0, 8, None) == E_SHAPE and fn(p, p, None, q, 8193, 8192, None) == E_SHAPE
        assert fn(None, p, None, q, 8, 8, None) == E_ARG and fn(p, p, None, None, 8, 8, None) == E_ARG
        assert fn(p, p, None, p, 8, 8, None) == E_ARG                       # in place: the warp gathers
        assert fn(p, p + 2, None, q, 8, 8, None) == E_ARG                   # the flow off the float grid
    for fn in (L.vst_temporal_l1_u8, L.vst_temporal_l1_f32):
        assert fn(p, q, None, 0, 8, p, None, p, None) == E_SHAPE
        assert fn(None, q, None, 8, 8, p, None, p, None) == E_ARG and fn(p, None, None, 8, 8, p, None, p, None) == E_ARG
        assert fn(p, q, None, 8, 8, None, None, p, None) == E_ARG and fn(p, q, None, 8, 8, p, None, None, None) == E_ARG
        assert fn(p, q, None, 8, 8, p + 4, None, p, None) == E_ARG          # loss3 off the 8-byte grid
        assert fn(p, q, None, 8, 8, p, p, p, None) == E_ARG                 # the warped frame over its source
    from vstnet_amd import temporal
    assert temporal.workspace_bytes(128, 260) == 24 * 17 and temporal.mean3([1.0, 2.0, 6.0]) == 3.0
    with pytest.raises(_lib.VstError):
        temporal.workspace_bytes(0, 8)


def test_front_end_argument_checks():
    import torch
    from vstnet_amd import temporal
    x, f = torch.zeros((3, 8, 9)), torch.zeros((2, 8, 9))
    with pytest.raises(ValueError):
        temporal.warp(x, f)                         # off the GPU: no fallback
    with pytest.raises(ValueError):
        temporal.temporal_loss(x, x.clone(), f)
    with pytest.raises(ValueError):
        temporal.fake_flow((200, 300), np.random.default_rng(0), device="cpu")
    with pytest.raises(ValueError):
        temporal.synthetic_clip(np.zeros((8, 8, 3), np.uint8), 3, device="cpu")
    grid, shifts = temporal.draw_fake_flow((37, 53), np.random.default_rng(3), 8, 10, cell=10)
    assert grid.shape == (3, 5, 2) and all(-10 <= s <= 10 and isinstance(s, int) for s in shifts)
    with pytest.raises(ValueError):
        temporal.draw_fake_flow((37, 53), np.random.default_rng(3), cell=40)


def test_import_path_without_cv2(monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)       # `import cv2` raises ImportError from here on
    sys.modules.pop("utils.TemporalLoss", None)
    import importlib
    mod = importlib.import_module("utils.TemporalLoss")
    assert "cv2" not in open(mod.__file__).read().replace("OpenCV", "")
    loss = mod.TemporalLoss(data_sigma=False, data_w=True, noise_level=0.002, motion_level=4, shift_level=3)
    assert (loss.data_sigma, loss.data_w, loss.noise_level, loss.motion_level, loss.shift_level) == (False, True, 0.002, 4, 3)
    for name in ("GenerateFakeFlow", "GenerateFakeData", "forward", "GaussianNoise"):
        assert callable(getattr(loss, name))
    import torch
    with pytest.raises(ValueError):
        mod.warp(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8))
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8))


# ---------------------------------------------------------------------------------------------------------------- the parser
def test_video_parser_errors(tmp_path, capsys):
    from PIL import Image
    import video_transfer
    img = tmp_path / "still.png"
    Image.fromarray(R.make_frame_u8(64, 96)).save(img)
    clip = tmp_path / "clip"
    clip.mkdir()
    for i in range(3):
        Image.fromarray(R.make_frame_u8(64, 96, i)).save(clip / f"{i:03d}.png")
    flows = tmp_path / "flows"
    flows.mkdir()
    base = ["--style", str(img), "--out_dir", str(tmp_path / "o"), "--synthetic_weights", "--frames_only", "--max_size", "96"]
    syn = base + ["--video", str(img), "--temporal", "--synthetic_motion", "4"]
    fromdir = base + ["--video", str(clip), "--temporal", "--flow_dir", str(flows)]
    cases = [
        (syn + ["--shard", "0/2"], "--shard"),
        (syn + ["--shard", "1/2"], "--shard"),
        (syn + ["--gpus", "2"], "--gpus"),
        (syn + ["--stub_stylise"], "--stub_stylise"),
        (syn + ["--out_pix_fmt", "yuv420p10le"], "high-bit-depth"),
        (syn + ["--upscale", "guided"], "--upscale guided"),
        (base + ["--video", str(img), "--temporal"], "exactly one source"),
        (syn + ["--flow_dir", str(flows)], "exactly one source"),
        (base + ["--video", str(clip), "--temporal", "--synthetic_motion", "4"], "single image"),
        (syn + ["--content_seg", str(img)], "--content_seg"),
        (syn + ["--content_seg_dir", str(clip)], "--content_seg_dir"),
        (syn + ["--strength_dir", str(clip)], "--strength_dir"),
        (base + ["--video", str(img), "--temporal", "--synthetic_motion", "1"], "at least 2"),
        (base + ["--video", str(clip), "--flow_dir", str(flows)], "belongs to --temporal"),
        (base + ["--video", str(img), "--synthetic_motion", "4"], "belongs to --temporal"),
        (syn + ["--flow_negate"], "--flow_negate"),
        # known only once the first frame has been seen: a written size that differs from the stylised one (the reference's
        # writer-size quirk at --max_size 80: a 96x64 frame is stylised at 80x52 and written at 80x64), and the number of flow
        # files.  (A synthetic clip is made at the stylised size, so it is written at that size whatever --max_size says.)
        (base[:-1] + ["80", "--video", str(clip), "--temporal", "--flow_dir", str(flows)], "stylised at 80x52 and written at 80x64"),
        (fromdir, "0 flow files"),
    ]
    for argv, what in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            video_transfer.main(argv)
        assert e.value.code == 2, argv
        assert what in capsys.readouterr().err, (argv, what)
    assert not (tmp_path / "o").exists() or not any(f.endswith(".csv") for _, _, fs in os.walk(tmp_path / "o") for f in fs)
