"""Guided upscale without a GPU: the yardstick (tests/guided_ref.py) against a brute-force version and against the properties a
guided filter must have, the float budget of the GPU comparisons, the scripts' parser cases and the C ABI's host-side checks.

Float budget, measured here (test_float_budget): max |guided_emul - guided_ref| over the GPU test's inputs (six shapes x two eps) = 1.963e-7; the GPU
comparisons allow 4 x that (profiles/guided_upscale.json, "emul_error")."""
import contextlib
import ctypes as C
import io
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest
from PIL import Image

import guided_ref as R
from vstnet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def noise_frame(hw, seed):
    return np.random.default_rng(seed).integers(0, 256, hw + (3,), dtype=np.uint8)


def test_ref_equals_brute_force():
    """7 x 9 working frame, r = 2 (every window clipped somewhere), non-integer ratios to 16 x 23"""
    G, S = noise_frame((7, 9), 1), noise_frame((16, 23), 2)
    P = np.random.default_rng(3).random((3, 7, 9))
    got, want = R.guided_ref(G, P, S, 2, 1e-3, False), R.brute_force(G, P, S, 2, 1e-3)
    assert got.shape == (3, 16, 23) and np.abs(got - want).max() < 1e-12
    assert R.guided_ref(G, P, S, 2, 1e-3, True).shape == (16, 23, 3)
    # the u8 form is the writer's epilogue of the float form
    assert np.array_equal(R.guided_ref(G, P, S, 2, 1e-3, True), np.moveaxis(R.quantise(want), 0, 2))


def test_quantise_is_the_writers_epilogue():
    q = np.array([-0.1, 0.0, 0.5 / 255, 0.999 / 255, 1.0 / 255, 254.999 / 255, 1.0, 1.7, np.nan])
    assert R.quantise(q).tolist() == [0, 0, 0, 0, 1, 254, 255, 255, 0]


def test_ref_affine_property():
    """white-noise guide (full-rank covariance), P = M I + c with a well-conditioned M, eps = 1e-9: the full-size result is
    M S / 255 + c.  (The ridge bias is eps / lambda_min ~ 1e-9 / 1e-2: far inside 1e-6.)"""
    G, S = noise_frame((20, 24), 4), noise_frame((47, 61), 5)
    M = np.array([[0.9, 0.1, -0.2], [0.05, 0.7, 0.2], [-0.1, 0.15, 0.8]])       # q = M i + c
    c = np.array([0.05, -0.02, 0.1])
    I = np.moveaxis(G / 255.0, 2, 0)
    P = np.einsum("ck,khw->chw", M, I) + c[:, None, None]
    want = np.einsum("ck,hwk->chw", M, S / 255.0) + c[:, None, None]
    assert np.abs(R.guided_ref(G, P, S, 3, 1e-9, False) - want).max() < 1e-6


def test_ref_identity_property_within_the_ridge_bias():
    """P = I gives S / 255 back up to the ridge: A = (Sigma + eps)^-1 Sigma = 1 - eps (Sigma + eps)^-1, so |A - 1|_2 <= eps /
    (lambda_min + eps) =: t, b = (1 - A)^T mean_I, and smoothing and sampling are convex combinations, so |q - s| <= t (|s| +
    |mean_I|) <= 2 sqrt(3) t.  With eps = 1e-7 and noise of variance >= 1e-2 that is below 1e-3."""
    G, S = noise_frame((20, 24), 6), noise_frame((47, 61), 7)
    r, eps = 3, 1e-7
    I = np.moveaxis(G / 255.0, 2, 0)
    assert I.var(axis=(1, 2)).min() >= 1e-2
    mI = R.box_mean(I, r)
    sigma = np.moveaxis(R.box_mean(I[:, None] * I[None, :], r) - mI[:, None] * mI[None, :], (0, 1), (2, 3))
    lam = np.linalg.eigvalsh(sigma).min()
    bound = 2.0 * np.sqrt(3.0) * eps / (lam + eps)
    print(f"identity: lambda_min {lam:.3e}, bound {bound:.3e}")
    assert bound < 1e-3
    err = np.abs(R.guided_ref(G, I, S, r, eps, False) - np.moveaxis(S / 255.0, 2, 0)).max()
    assert err <= bound + 1e-12, (err, bound)


def test_ref_constant_property():
    G, S = noise_frame((12, 16), 8), noise_frame((30, 41), 9)
    P = np.broadcast_to(np.array([0.25, 0.5, 0.75])[:, None, None], (3, 12, 16))
    got = R.guided_ref(G, P, S, 4, 1e-3, False)
    assert np.abs(got - np.array([0.25, 0.5, 0.75])[:, None, None]).max() < 1e-6


def test_emul_is_the_ref_with_fp32_storage():
    """same formulas: on a case whose numbers are exact in fp32 both give the same result"""
    G = np.full((8, 8, 3), 51, np.uint8)                    # 0.2: constant guide, zero covariance -> A = 0, b = mean_p
    P = np.full((3, 8, 8), 0.5)
    S = noise_frame((16, 16), 10)
    assert np.array_equal(R.guided_emul(G, P, S, 2, 1e-3, False), R.guided_ref(G, P, S, 2, 1e-3, False))


def test_float_budget():
    """max |guided_emul - guided_ref| over the GPU test's inputs, printed; the value recorded in profiles/guided_upscale.json is
    this measurement (a coefficient is a few units large, so a few fp32 roundings of 6e-8 each)"""
    e = R.emul_error()
    print(f"guided upscale: max |emul - ref| = {e:.3e}, float budget {R.float_budget():.3e}")
    assert 0.0 < e < 1e-5
    rec = json.load(open(os.path.join(REPO, "profiles", "guided_upscale.json")))["emul_error"]
    assert 0.8 * rec <= e <= 1.25 * rec, (e, rec)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_workspace_bytes_and_bad_radius_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.vst_version() >= 116 and _lib.GUIDED_MAX_RADIUS == 8
    n = C.c_size_t(0)
    assert L.vst_guided_workspace_bytes(720, 1280, 4, C.byref(n)) == 0 and n.value == 720 * 1280 * 33 * 8
    E_ARG, E_SHAPE, E_WS, p = -1, -2, -4, 4096      # (a non-null address: nothing dereferences it before the checks)
    for r in (0, 9, -1):
        assert L.vst_guided_workspace_bytes(64, 64, r, C.byref(n)) == E_SHAPE
        assert L.vst_guided_fit(p, p, 64, 64, r, 1e-3, p, p, None) == E_SHAPE
    assert L.vst_guided_workspace_bytes(64, 64, 4, None) == E_ARG
    assert L.vst_guided_workspace_bytes(0, 64, 4, C.byref(n)) == E_ARG
    assert L.vst_guided_workspace_bytes(8192, 8192, 4, C.byref(n)) == E_SHAPE          # 48 h w passes 2^31
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        assert L.vst_guided_fit(p, p, 64, 64, 4, eps, p, p, None) == E_ARG
    assert L.vst_guided_fit(None, p, 64, 64, 4, 1e-3, p, p, None) == E_ARG
    assert L.vst_guided_fit(p, p, 64, 64, 4, 1e-3, p, None, None) == E_WS
    for fn in (L.vst_guided_apply_u8, L.vst_guided_apply_f32):
        assert fn(p, 64, 64, p, 63, 64, p, None) == E_SHAPE             # H < h
        assert fn(p, 64, 64, p, 64, 63, p, None) == E_SHAPE             # W < w
        assert fn(None, 64, 64, p, 64, 64, p, None) == E_ARG
        assert fn(p, 64, 64, p, 0, 64, p, None) == E_ARG
    # byte offsets past 2^31: 3 H W for the u8 form, 12 H W for the f32 form
    assert L.vst_guided_apply_u8(p, 64, 64, p, 32768, 32768, p, None) == E_SHAPE
    assert L.vst_guided_apply_f32(p, 64, 64, p, 16384, 16384, p, None) == E_SHAPE
    from vstnet_amd import guided
    assert guided.workspace_bytes(24, 36, 1) == 24 * 36 * 33 * 8
    with pytest.raises(_lib.VstError):
        guided.workspace_bytes(24, 36, 9)


# ---------------------------------------------------------------------------------------------------------------- the scripts
class _Done:
    def __init__(self, returncode, stdout, stderr):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr


def _run(main, args):
    """script.main(args) in this process, reporting the exit status, stdout and stderr as a command line would give them (every
    case below ends in the parser, or runs the host rehearsal --stub_stylise: no GPU)"""
    out, err, rc = io.StringIO(), io.StringIO(), 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            main(list(args))
        except SystemExit as e:
            rc = e.code if isinstance(e.code, int) else 1
        except Exception:       # noqa: BLE001 - what the interpreter would print before it exits with status 1
            traceback.print_exc()
            rc = 1
    return _Done(rc, out.getvalue(), err.getvalue())


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("guided")
    os.makedirs(d / "frames")
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (56, 40, 3), dtype=np.uint8)).save(d / "frames" / ("%03d.png" % i))
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(d / "s.png")
    return d


def test_video_parser_cases(clip, tmp_path):
    import video_transfer
    from yuv16_ref import DeepYuvSpec, write_raw
    from vstnet_amd import yuv
    out = ["--out_dir", str(tmp_path / "o")]
    head = ["--video", str(clip / "frames"), "--style", str(clip / "s.png"), "--max_size", "32"] + out
    run = lambda a: _run(video_transfer.main, a)          # noqa: E731
    # --resize host, given or as the default: the error names --resize device
    for extra in (["--resize", "host"], []):
        p = run(head + ["--upscale", "guided"] + extra)
        assert p.returncode == 2 and "--resize device" in p.stderr, p.stderr[-500:]
    # a high-bit-depth output, then a high-bit-depth input
    p = run(head + ["--upscale", "guided", "--resize", "device", "--out_pix_fmt", "yuv420p10le"])
    assert p.returncode == 2 and "high-bit-depth" in p.stderr, p.stderr[-500:]
    spec = DeepYuvSpec("420mpeg2", "bt601", "limited", 10)
    yy, xx = np.mgrid[0:56, 0:40]
    write_raw(str(tmp_path / "deep.yuv"), [yuv.rgb_to_yuv16_host(np.stack([xx / 40, yy / 56, (xx + yy) / 96], axis=-1), spec)])
    p = run(["--video", str(tmp_path / "deep.yuv"), "--pix_fmt", "yuv420p10le", "--video_size", "40x56", "--style",
             str(clip / "s.png"), "--max_size", "32", "--resize", "device", "--upscale", "guided"] + out)
    assert p.returncode == 2 and "high-bit-depth" in p.stderr, p.stderr[-500:]
    # the artistic model is not locally affine
    p = run(head + ["--upscale", "guided", "--resize", "device", "--mode", "artistic"])
    assert p.returncode == 2 and "artistic" in p.stderr and "locally affine" in p.stderr, p.stderr[-500:]
    # the radius and the ridge
    for flag, bad in (("--upscale_radius", "0"), ("--upscale_radius", "9"), ("--upscale_eps", "0"), ("--upscale_eps", "-1e-3")):
        p = run(head + ["--upscale", "guided", "--resize", "device", flag, bad])
        assert p.returncode == 2 and flag in p.stderr, (flag, bad, p.stderr[-500:])
    p = run(head + ["--upscale", "nearest"])
    assert p.returncode == 2 and "invalid choice" in p.stderr
    # the host rehearsal stylises nothing: no guided step
    p = run(head + ["--upscale", "guided", "--resize", "device", "--stub_stylise"])
    assert p.returncode == 2 and "--stub_stylise" in p.stderr, p.stderr[-500:]
    assert not os.path.exists(tmp_path / "o") or not any(f.endswith(".png") for _, _, fs in os.walk(tmp_path / "o") for f in fs)
    # nothing to upscale (a 40x56 frame passes --max_size 64 unchanged): one line on stderr, and the plain path carries on -
    # even with --resize host, which the plain path takes
    base = ["--video", str(clip / "frames"), "--style", str(clip / "s.png"), "--max_size", "64", "--stub_stylise", "--frames_only"]
    p = run(base + ["--upscale", "guided", "--out_dir", str(tmp_path / "g")])
    assert p.returncode == 0 and "nothing to upscale" in p.stderr, p.stderr[-800:]
    q = run(base + ["--out_dir", str(tmp_path / "b")])
    assert q.returncode == 0 and "upscale" not in q.stderr
    files = lambda d: sorted(os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith(".png"))    # noqa: E731
    got, want = files(tmp_path / "g"), files(tmp_path / "b")
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert open(a, "rb").read() == open(b, "rb").read()


def test_video_parser_error_from_the_command_line(clip, tmp_path):
    """one case as a real command: exit status 2 and the message on stderr, before any GPU work"""
    p = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py"), "--video", str(clip / "frames"), "--style",
                        str(clip / "s.png"), "--max_size", "32", "--out_dir", str(tmp_path / "o"), "--upscale", "guided",
                        "--resize", "device", "--mode", "artistic"], capture_output=True, text=True, cwd=REPO)
    assert p.returncode == 2 and "--upscale guided" in p.stderr and "artistic" in p.stderr, p.stderr[-500:]


def test_image_parser_cases(clip, tmp_path):
    import image_transfer
    head = ["--content", str(clip / "frames" / "000.png"), "--style", str(clip / "s.png"), "--out_dir", str(tmp_path / "o"),
            "--synthetic_weights", "--upscale", "guided"]
    run = lambda a: _run(image_transfer.main, a)          # noqa: E731
    p = run(head + ["--max_size", "32", "--mode", "artistic"])
    assert p.returncode == 2 and "artistic" in p.stderr, p.stderr[-500:]
    for flag, bad in (("--upscale_radius", "9"), ("--upscale_eps", "0")):
        p = run(head + ["--max_size", "32", flag, bad])
        assert p.returncode == 2 and flag in p.stderr, p.stderr[-500:]
    # the tiled route: an image past the whole-frame guard (only its header is read here)
    Image.new("1", (8200, 8200)).save(tmp_path / "huge.png")
    p = run(["--content", str(tmp_path / "huge.png")] + head[2:] + ["--max_size", "16384"])
    assert p.returncode == 2 and "tiled route" in p.stderr and "--upscale guided" in p.stderr, p.stderr[-500:]
