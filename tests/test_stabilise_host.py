"""The temporal stabiliser without a GPU: the C ABI's host-side checks, the front end's refusals, stabilise.csv, the parser errors
of video_transfer.py --stabilise, and what the numpy statement the device is held to (tests/stabilise_ref.py) does on its own -
dead pixels, the step limit, the fall-off of the weight, and two constructed clips on which it must more than halve the warping
error of every frame pair."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stabilise_ref as S
from vstnet_amd import _lib


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.vst_version() >= 121
    header = open(os.path.join(_lib.REPO_DIR, "include", "vstnet.h")).read()
    assert "Stabiliser (version 121" in header and "int vst_stabilise_u8(" in header
    assert "vst_stabilise_u8" in _lib.EXPORTS and hasattr(L, "vst_stabilise_u8")
    E_ARG, E_SHAPE = -1, -2
    # non-null addresses that nothing dereferences, far apart: every refusal comes before the launch
    ci, pi, co, pw, fl, va, wr = (k << 24 for k in range(1, 8))

    def call(ptrs=(ci, pi, co, pw, fl, va, wr), h=16, w=16, gain=0.7, sigma=8.0, limit=24.0):
        return L.vst_stabilise_u8(*ptrs[:6], h, w, gain, sigma, limit, ptrs[6], None)

    for k in (0, 1, 2, 3, 4, 6):                    # every pointer but valid
        ptrs = [ci, pi, co, pw, fl, va, wr]
        ptrs[k] = None
        assert call(tuple(ptrs)) == E_ARG, k
    for h, w in ((0, 16), (16, 0), (-1, 4), (8193, 8192)):
        assert call(h=h, w=w) == E_SHAPE, (h, w)
    for gain in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert call(gain=gain) == E_ARG, gain
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert call(sigma=sigma) == E_ARG, sigma
    for limit in (-1e-9, float("nan"), float("inf")):
        assert call(limit=limit) == E_ARG, limit
    assert call((ci, pi, co, pw, fl + 2, va, wr)) == E_ARG                  # the flow off the float grid
    n = 16 * 16 * 3
    for alias in (pw, co, pw + n - 1, co - n + 1, pi, ci, fl, va):          # `written` over an input, wholly or in part
        assert call((ci, pi, co, pw, fl, va, alias)) == E_ARG, hex(alias)


def test_front_end_argument_checks():
    import torch
    from vstnet_amd import stabilise as M
    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    f = torch.zeros((2, 16, 16), dtype=torch.float32)
    with pytest.raises(ValueError):
        M.stabilise(x, x.clone(), x.clone(), x.clone(), f)      # off the GPU: no fallback
    with pytest.raises(ValueError):
        M.Stabiliser((16, 16), device="cpu")
    for bad in (dict(gain=0.0), dict(gain=1.0), dict(sigma=0.0), dict(limit=-1.0), dict(gain=float("nan"))):
        with pytest.raises(ValueError):
            M.check_params(**{**M.DEFAULTS, **bad})
    assert M.check_params(**M.DEFAULTS) == (0.7, 8.0, 24.0) and M.DEFAULTS == S.DEFAULTS
    assert "STARTING VALUES" in M.__doc__ and "unmeasured" in M.__doc__


def test_stabilise_csv(tmp_path):
    from vstnet_amd import flowfiles as FF
    rows = {1: (0.2, 0.1), 2: (0.4, float("nan")), 3: (0.25, 0.125)}
    p = FF.write_stabilise_csv(tmp_path / FF.STABILISE_CSV_NAME, rows, 5)
    assert os.path.basename(p) == "stabilise.csv"
    assert open(p).read().splitlines() == ["0,,", "1,0.2,0.1", "2,0.4,", "3,0.25,0.125", "4,,"]
    back = FF.read_stabilise_csv(p)
    assert back[0] == (None, None) and back[1] == (0.2, 0.1) and back[2] == (0.4, None)
    assert open(FF.write_stabilise_csv(tmp_path / "again.csv", back), "rb").read() == open(p, "rb").read()
    line = FF.stabilise_summary(back)
    assert "2 frame pairs" in line and line.endswith("written / decoded 0.500")
    assert FF.stabilise_summary({}) == "stabilise: no frame pairs"
    open(tmp_path / "bad.csv", "w").write("0,1.0\n")
    with pytest.raises(ValueError, match="bad.csv line 1"):
        FF.read_stabilise_csv(tmp_path / "bad.csv")


# ---------------------------------------------------------------------------------------------------------------- the script
def test_video_parser_errors(tmp_path):
    """Each command line in a process of its own: exit status 2 and the message, before anything is read or written."""
    from PIL import Image
    img = tmp_path / "still.png"
    Image.fromarray(S.constructed_clip("static", n=1)[0][0]).save(img)
    clip = tmp_path / "clip"
    clip.mkdir()
    segs = tmp_path / "segs"
    segs.mkdir()
    base = ["--style", str(img), "--out_dir", str(tmp_path / "o"), "--synthetic_weights", "--frames_only", "--max_size", "64",
            "--video", str(clip)]
    est = base + ["--temporal", "--estimate_flow"]
    cases = [
        (base + ["--stabilise"], "--stabilise belongs to --temporal"),
        (est + ["--stabilise", "--content_seg_dir", str(segs)], "--content_seg_dir"),
        (est + ["--stabilise", "--auto_seg"], "--auto_seg"),
        (est + ["--stabilise", "0"], "--stabilise GAIN"),
        (est + ["--stabilise", "1"], "--stabilise GAIN"),
        (est + ["--stabilise", "--stabilise_sigma", "0"], "--stabilise_sigma"),
        (est + ["--stabilise", "--stabilise_limit", "-1"], "--stabilise_limit"),
        (est + ["--stabilise", "--shard", "0/2"], "--shard"),
    ]
    script = os.path.join(_lib.REPO_DIR, "video_transfer.py")
    procs = [subprocess.Popen([sys.executable, script] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              cwd=_lib.REPO_DIR) for argv, _ in cases]
    for (argv, what), p in zip(cases, procs):
        _, err = p.communicate()
        assert p.returncode == 2, (argv, p.returncode, err[-400:])
        assert "error:" in err and what in err, (argv, what, err[-400:])
    assert not (tmp_path / "o").exists()


# ---------------------------------------------------------------------------------------------------------------- the reference
def frames(h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]


def test_dead_pixels_return_cur_out():
    h, w = 9, 13
    ci, pi, co, pw = frames(h, w, 0)
    flow = np.zeros((2, h, w), np.float32)
    flow[0, :, 0] = 0.5                             # one column points out on the left
    flow[1, h - 1, :] = -0.25                       # the last row points out below
    flow[0, 2, 3], flow[1, 3, 4], flow[0, 4, 5], flow[1, 5, 6] = np.nan, np.inf, -np.inf, np.nan
    valid = np.ones((h, w), np.uint8)
    valid[6, 7:10] = 0
    dead = np.zeros((h, w), bool)
    dead[:, 0] = dead[h - 1, :] = dead[2, 3] = dead[3, 4] = dead[4, 5] = dead[5, 6] = True
    got = S.stabilise(ci, pi, co, pw, flow)
    assert np.array_equal(got[dead], co[dead]) and not np.array_equal(got[~dead], co[~dead])
    dead[6, 7:10] = True
    got = S.stabilise(ci, pi, co, pw, flow, valid)
    assert np.array_equal(got[dead], co[dead]) and not np.array_equal(got[~dead], co[~dead])
    # a flow that is out of the frame, or not a number, everywhere: the frame as it came
    for v in (np.nan, np.inf, -np.inf, 1000.0):
        assert np.array_equal(S.stabilise(ci, pi, co, pw, np.full((2, h, w), v, np.float32)), co)


@pytest.mark.parametrize("limit", (0.0, 0.5, 3.0, 24.0, 24.5))
def test_step_limit(limit):
    h, w = 17, 19
    ci, pi, co, pw = frames(h, w, 1)
    flow = np.random.default_rng(2).normal(0.0, 1.5, (2, h, w)).astype(np.float32)
    got = S.stabilise(ci, ci, co, pw, flow * 0, gain=0.99, limit=limit)      # (the input unchanged: the weight is the gain)
    step = np.abs(got.astype(np.int64) - co.astype(np.int64))
    assert step.max() <= np.ceil(limit) and (limit == 0.0 or step.max() >= np.floor(limit))
    got = S.stabilise(ci, pi, co, pw, flow, limit=limit)
    assert np.abs(got.astype(np.int64) - co.astype(np.int64)).max() <= np.ceil(limit)


def test_changed_input_moves_nothing():
    """An input residual of 100 levels on all channels: wgt = 0.7 / (1 + 10000 / 64) = 0.0045, at most 1.1 levels of a 255-level
    difference: no byte moves by more than 2."""
    h, w = 12, 16
    rng = np.random.default_rng(3)
    pi = rng.integers(0, 156, (h, w, 3), dtype=np.uint8)
    ci = pi + 100
    co = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for pw in (np.zeros_like(co), np.full_like(co, 255), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)):
        got = S.stabilise(ci, pi, co, pw, np.zeros((2, h, w), np.float32))
        assert np.abs(got.astype(np.int64) - co.astype(np.int64)).max() <= 2
    # and where the input did not change the output follows the written frame: a gain's worth of the way
    got = S.stabilise(pi, pi, co, np.full_like(co, 128), np.zeros((2, h, w), np.float32), limit=255.0)
    want = np.rint(co + 0.7 * (128.0 - co))
    assert np.array_equal(got, want.astype(np.uint8))


@pytest.mark.parametrize("kind", ("static", "moving"))
def test_constructed_clips_halve_the_warping_error(kind):
    """48x64, 8 frames, seed 0, noise of 3 levels on the inputs and on the stylised frames, a gain flicker of 6 %: with the
    defaults the bilinear warping error of the stabilised sequence is below 0.5 of the raw one for EVERY frame pair.  (The numpy
    statement gives 0.18 .. 0.44 on both clips; the first pair, which has no history behind it, is the largest.)"""
    inputs, stylised, flows = S.constructed_clip(kind, n=8, h=48, w=64, seed=0, noise=3.0, flicker=0.06)
    written = S.run_sequence(inputs, stylised, flows)
    assert np.array_equal(written[0], stylised[0])
    ratios = []
    for t in range(1, 8):
        raw = S.warping_error(stylised[t - 1], stylised[t], flows[t])
        out = S.warping_error(written[t - 1], written[t], flows[t])
        ratios.append(out / raw)
        assert raw > 3.0                            # (there is flicker to damp on every pair)
    print(kind, ["%.3f" % r for r in ratios])
    assert max(ratios) < 0.5, ratios
