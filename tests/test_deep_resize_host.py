"""The deep resize without a GPU ("Deep resize"): the double table against a numpy restatement and against
Pillow's 22-bit one, img_resize_float against Pillow itself within the bound tests/deep_resize_ref.py derives, the C ABI's
argument checks, the header against the export table, and `video_transfer.py --stub_stylise` on deep clips of any size."""
import contextlib
import ctypes as C
import io
import os
import re
import traceback

import numpy as np
import pytest
from PIL import Image

import deep_resize_ref as R
from deep_resize_ref import DeepYuvSpec
from vstnet_amd import _lib
from vstnet_amd import resize as RS
from vstnet_amd.rawyuv import RawYuvClip, merge_parts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = sorted({(n_in, n_out) for W, H, m in R.SHAPES for _, n_in, n_out in R.float_passes((W, H), m, 4)} | {(64, 4), (7, 7), (5, 3)})


# -------------------------------------------------------------------------------------------------------------------- tables
def cubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def table_by_hand(in_size, out_size):
    """Pillow's precompute_coeffs in Python floats (IEEE doubles, no contraction), operation for operation"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, w = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ksize), np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        k = [cubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in k:
            ww += v
        w[xx, :n] = [v / ww for v in k] if ww != 0.0 else k
        bounds[xx] = (xmin, n)
    return ksize, bounds, w


@pytest.mark.parametrize("in_size,out_size", AXES)
def test_f64_table_equals_the_formula_and_rounds_to_pillows(in_size, out_size):
    ks, bounds, w = RS.coeffs_f64(in_size, out_size)
    ks_h, bounds_h, w_h = table_by_hand(in_size, out_size)
    assert ks == ks_h and w.dtype == np.float64 and np.array_equal(bounds, bounds_h)
    assert np.array_equal(w.view(np.int64), w_h.view(np.int64)), "a weight differs in its last bit"
    ks8, bounds8, kk = RS.coeffs_u8(in_size, out_size)
    assert ks8 == ks and np.array_equal(bounds8, bounds)
    scaled = w * float(1 << 22)
    assert np.array_equal(np.where(w < 0, -0.5 + scaled, 0.5 + scaled).astype(np.int32), kk)   # ((int): towards zero)


def test_f64_table_protocol_and_errors():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    ks = C.c_int(0)
    assert L.vst_resize_coeffs_f64(97, 64, C.byref(ks), None, None) == 0 and ks.value == 2 * 4 + 1
    assert L.vst_resize_coeffs_f64(97, 64, None, None, None) == -1
    assert L.vst_resize_coeffs_f64(0, 64, C.byref(ks), None, None) == -1
    assert L.vst_resize_coeffs_f64(1025, 64, C.byref(ks), None, None) == -2
    assert L.vst_resize_coeffs_f64(1024, 64, C.byref(ks), None, None) == 0 and ks.value == 65


# ------------------------------------------------------------------------------------------------------------ against Pillow
@pytest.mark.parametrize("W,H,max_size", R.SHAPES)
def test_img_resize_float_against_pillow(W, H, max_size):
    """bytes from 48..207 (full-range noise does not qualify: Pillow clamps to 0..255 after each pass)"""
    from utils.utils import img_resize
    a = np.random.default_rng(W + H).integers(48, 208, (H, W, 3), dtype=np.uint8)
    want = np.asarray(img_resize(Image.fromarray(a), max_size, down_scale=4)).astype(np.float64)
    got = RS.img_resize_float(a.astype(np.float64), max_size, 4)
    assert got.shape == want.shape == RS.img_resize_size((W, H), max_size, 4)[::-1] + (3,)
    diff, bound = float(np.abs(got - want).max()), R.pillow_bound((W, H), max_size)
    print(f"{W}x{H} to {max_size}: {diff:.3f} from Pillow, bound {bound:.3f}")
    assert diff <= bound
    # the passes are linear: the scale is the caller's
    assert np.allclose(RS.img_resize_float(a / 255.0, max_size, 4) * 255.0, got, rtol=0, atol=1e-10)


def test_passes_and_limits():
    assert R.float_passes((97, 55), 64, 4) == [(1, 97, 64), (0, 55, 36)]
    assert R.float_passes((42, 56), 64, 4) == [(1, 42, 40)]
    assert R.float_passes((40, 58), 64, 4) == [(0, 58, 56)]
    assert R.float_passes((160, 140), 12, 4) == [(1, 160, 12), (0, 140, 10), (0, 10, 8)]
    assert R.float_passes((301, 77), 150, 4) == [(1, 301, 150), (0, 77, 38), (1, 150, 148), (0, 38, 36)]
    assert R.float_passes((40, 56), 64, 4) == []
    with pytest.raises(_lib.VstError, match="16"):
        RS.img_resize_float(np.zeros((8, 2000, 3)), 64, 4)
    assert 1e-7 < R.kernel_tolerance((301, 77), 150) < 1e-6 and R.kernel_tolerance((40, 56), 64) == 2.0 ** -24


# -------------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_refuses_bad_arguments_before_any_launch():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    E_ARG, E_SHAPE, p = -1, -2, 4096            # (a non-null, 8-byte aligned address: nothing dereferences it before the checks)

    def call(Hs=55, Ws=97, depth=10, layout=2, matrix=1, rng=0, steps=((64, 36), (64, 36)), ptrs=(p, p, p, p, p, p, p), nsteps=None):
        arr = (C.c_int * max(1, 2 * len(steps)))(*[v for wh in steps for v in wh])
        return L.vst_yuv16_img_resize_f32(ptrs[0], ptrs[1], ptrs[2], Hs, Ws, depth, layout, matrix, rng,
                                          len(steps) if nsteps is None else nsteps, arr, ptrs[3], ptrs[4], ptrs[5], ptrs[6], None)
    for k in (0, 1, 2, 3, 4, 5):                # y, u, v, tables, work, out_f32 (out_u8 may be NULL, checked on the GPU)
        a = [p] * 7
        a[k] = None
        assert call(ptrs=tuple(a)) == E_ARG, k
    for kw in (dict(depth=8), dict(depth=17), dict(layout=4), dict(matrix=2), dict(rng=-1), dict(Hs=0), dict(Ws=-1), dict(nsteps=5),
               dict(nsteps=-1), dict(steps=((64, 0),)), dict(ptrs=(p, p, p, p + 4, p, p, p)),
               dict(Hs=8193, Ws=8192, steps=((8192, 8192),))):
        assert call(**kw) == E_ARG, kw
    for kw in (dict(Ws=1025, steps=((64, 36),)), dict(Hs=577, steps=((64, 36),)), dict(steps=((98, 36),)), dict(steps=((64, 56),)),
               dict(steps=((64, 36), (64, 40)))):
        assert call(**kw) == E_SHAPE, kw
    n = C.c_size_t(0)
    steps = (C.c_int * 4)(64, 36, 64, 36)
    assert L.vst_yuv16_img_resize_workspace_bytes(55, 97, 2, steps, C.byref(n)) == 0 and n.value == 4 * 3 * 55 * 64
    assert L.vst_yuv16_img_resize_workspace_bytes(55, 97, 2, steps, None) == E_ARG
    steps = (C.c_int * 2)(40, 56)
    assert L.vst_yuv16_img_resize_workspace_bytes(58, 40, 1, steps, C.byref(n)) == 0 and n.value == 4 * 3 * 58 * 40
    assert L.vst_yuv16_img_resize_workspace_bytes(56, 42, 1, steps, C.byref(n)) == 0 and n.value == 0
    steps = (C.c_int * 2)(64, 36)
    assert L.vst_yuv16_img_resize_workspace_bytes(55, 1025, 1, steps, C.byref(n)) == E_SHAPE


def test_header_and_exports_agree():
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|int64_t|const char\*)\s+(vst_\w+)\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS)
    for name in ("vst_resize_coeffs_f64", "vst_yuv16_img_resize_workspace_bytes", "vst_yuv16_img_resize_f32"):
        assert name in declared
    assert "Deep resize (version 115" in hdr


# ---------------------------------------------------------------------------------------------------------------- the script
class _Done:
    def __init__(self, returncode, stdout, stderr):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr


def _run(args):
    """video_transfer.main(args) in this process (--stub_stylise: no GPU), reporting the exit status, stdout and stderr as a
    command line would give them"""
    import video_transfer
    out, err, rc = io.StringIO(), io.StringIO(), 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            video_transfer.main(list(args))
        except SystemExit as e:
            rc = e.code if isinstance(e.code, int) else 1
        except Exception:       # noqa: BLE001 - what the interpreter would print before it exits with status 1
            traceback.print_exc()
            rc = 1
    return _Done(rc, out.getvalue(), err.getvalue())


SPEC0 = DeepYuvSpec("420mpeg2", "bt601", "limited", 10)


def smooth_frame(H, W, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([(xx + seed) / (W + seed), yy / H, (xx + yy) / (W + H - 1.0)], axis=-1)
    return R.rgb_to_yuv16_host(rgb, SPEC0)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """a landscape 97x55 clip (the writer-size rule writes it at 64x55, not at the stylised 64x36) and a portrait 55x97 one (both
    sizes 36x64)"""
    d = tmp_path_factory.mktemp("deep")
    Image.fromarray(np.zeros((20, 20, 3), np.uint8)).save(d / "s.png")
    out = {}
    for name, (W, H) in (("wide", (97, 55)), ("tall", (55, 97))):
        frames = [smooth_frame(H, W, i) for i in range(3)]
        R.write_raw(str(d / (name + ".yuv")), frames)
        out[name] = (W, H, frames, ["--video", str(d / (name + ".yuv")), "--style", str(d / "s.png"), "--stub_stylise", "--max_size",
                                    "64", "--pix_fmt", "yuv420p10le", "--video_size", "%dx%d" % (W, H)])
    return d, out


def expected(frame, W, H, written_wh):
    """the bytes of a stylised frame under --stub_stylise: rgb_to_yuv16_host of img_resize_float of yuv16_to_rgb_float, with the
    rehearsal of the resize to the written size in between where that differs from the stylised size"""
    x = R.reference(frame, H, W, SPEC0, 64)
    if (x.shape[1], x.shape[0]) != tuple(written_wh):
        x = RS.resize_float(x, (written_wh[1], written_wh[0]))
    return R.rgb_to_yuv16_host(x, SPEC0)


def test_script_resizes_a_deep_clip_with_resize_device(clips):
    import video_transfer
    d, c = clips
    for name, sty_wh in (("tall", (36, 64)), ("wide", (64, 36))):
        W, H, frames, base = c[name]
        assert RS.img_resize_size((W, H), 64, 4) == sty_wh
        wsz = video_transfer.writer_size((W, H), 64)
        p = _run(base + ["--resize", "device", "--out_dir", str(d / name)])
        assert p.returncode == 0, p.stderr[-2000:]
        path = d / name / ("%s_s_%dx%d_yuv420p10le.yuv" % (name, wsz[0], wsz[1]))
        assert "Save stylized video at %s" % path in p.stdout
        out = RawYuvClip(str(path), wsz[0], wsz[1], "yuv420p10le")
        assert len(out) == 3
        for i in range(3):
            assert np.array_equal(out[i], expected(frames[i], W, H, wsz)), (name, i)
    # the portrait clip is written at its stylised size: the frames are the reference's bytes, nothing in between
    W, H, frames, _ = c["tall"]
    assert video_transfer.writer_size((W, H), 64) == (36, 64)
    out = RawYuvClip(str(d / "tall" / "tall_s_36x64_yuv420p10le.yuv"), 36, 64, "yuv420p10le")
    assert np.array_equal(out[1], R.reference_frame(frames[1], H, W, SPEC0, 64, SPEC0))


def test_script_refuses_without_resize_device_and_past_the_limit(clips, tmp_path):
    d, c = clips
    W, H, frames, base = c["wide"]
    for extra in ([], ["--resize", "host"]):
        p = _run(base + extra + ["--out_dir", str(tmp_path / "e")])
        assert p.returncode == 2 and "97x55" in p.stderr and "--max_size" in p.stderr and "multiples of 4" in p.stderr \
            and "not built yet" in p.stderr and "--resize device" in p.stderr, p.stderr[-500:]
    # a shrink above 16: 97 -> 4
    p = _run(base[:-6] + ["--max_size", "4", "--pix_fmt", "yuv420p10le", "--video_size", "97x55", "--resize", "device", "--out_dir",
                          str(tmp_path / "e")])
    assert p.returncode == 2 and "16" in p.stderr and "shrink" in p.stderr, p.stderr[-500:]
    assert not os.path.exists(tmp_path / "e") or not [f for f in os.listdir(tmp_path / "e") if f.endswith(".yuv")]


def test_script_shards_equal_one_process(clips):
    d, c = clips
    W, H, frames, base = c["wide"]
    base = base + ["--resize", "device"]
    p = _run(base + ["--out_dir", str(d / "whole")])
    assert p.returncode == 0, p.stderr[-2000:]
    name = "wide_s_64x55_yuv420p10le.yuv"
    one = open(d / "whole" / name, "rb").read()
    assert len(one) == 3 * SPEC0.frame_bytes(55, 64)
    for r in range(2):
        p = _run(base + ["--out_dir", str(d / "sh"), "--shard", "%d/2" % r])
        assert p.returncode == 0, p.stderr[-2000:]
    parts = [str(d / "sh" / "wide_s" / ("part_%d.yuv" % r)) for r in range(2)]
    merged = merge_parts(str(d / "sh" / name), parts, 3, SPEC0.frame_bytes(55, 64))
    assert open(merged, "rb").read() == one
    p = _run(base + ["--out_dir", str(d / "g2"), "--gpus", "2"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(d / "g2" / name, "rb").read() == one
