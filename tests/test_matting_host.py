"""The affinity loss without a GPU: the yardstick (tests/matting_ref.py) against the reference's own matrix
(tests/golden/matting.npz, written by tests/make_matting_golden.py), its float budget, its properties, the reference's import
path, the C ABI's host-side checks and the join of the shards' affinity files.

Against the golden, measured here (test_ref_against_the_reference): the loss deviates by at most 1.60e-8 relative, the doubled
gradient by at most 7.78e-8 of its largest entry - the reference's cast of L to float32, which depends on the image; the tolerance
is 4 x the largest deviation seen, golden_tolerance().

Float budget, measured here (test_float_budget): fp64 against longdouble over CASES x the three forms of x, the loss relative to
sum_k n var_k(x) / (h w), the gradient absolute: 5.33e-15 and 3.28e-17 against the L D L^T twin, 2.07e-7 and 1.85e-10 against the
issue's adjugate twin (the adjugate's own loss on the step case); the device budgets are 16 x the smaller of each pair."""
import ctypes as C
import os

import numpy as np
import pytest

import matting_ref as R
from vstnet_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED_GOLDEN = (1.601e-8, 7.785e-8)     # largest deviation from the golden: loss (relative), gradient (of its largest entry)
GOLD = ("noise", "ramp")


def _golden_deviations():
    gold = np.load(os.path.join(HERE, "golden", "matting.npz"))
    out = []
    for name in GOLD:
        for r in (1, 2):
            res = R.matting(gold[f"{name}_guide"], gold[f"{name}_x"], r, float(gold["eps"]))
            want_l, want_g = float(gold[f"{name}_r{r}_loss"]), gold[f"{name}_r{r}_grad2"]
            out.append((name, r, abs(float(res["loss"].sum()) - want_l) / want_l,
                        float(np.abs(res["grad"] - want_g).max() / np.abs(want_g).max()),
                        abs(float(res["closed"].sum()) - want_l) / want_l))
    return out


def golden_tolerance():
    """(loss relative, gradient relative to its largest entry): 4 x the largest deviation of the yardstick from the golden, as
    measured and recorded in MEASURED_GOLDEN (test_ref_against_the_reference holds the record to the measurement)"""
    return 4.0 * MEASURED_GOLDEN[0], 4.0 * MEASURED_GOLDEN[1]


def test_ref_against_the_reference():
    """The gap is the reference's float32 cast of L (2^-24 = 6e-8 per entry) and depends on the image: every golden case lies
    within 4 x the largest deviation seen, and that largest deviation is the recorded one."""
    dev = _golden_deviations()
    tl, tg = golden_tolerance()
    for name, r, el, eg, ec in dev:
        print(f"golden {name} r={r}: loss {el:.3e} relative (per-window form {ec:.3e}), gradient {eg:.3e} of its largest entry")
        assert el <= tl and ec <= tl and eg <= tg
    worst = max(x[2] for x in dev), max(x[3] for x in dev)
    print(f"golden: largest deviation loss {worst[0]:.3e}, gradient {worst[1]:.3e}; tolerance {tl:.3e}, {tg:.3e}")
    assert 0.8 * MEASURED_GOLDEN[0] <= worst[0] <= 1.25 * MEASURED_GOLDEN[0]
    assert 0.8 * MEASURED_GOLDEN[1] <= worst[1] <= 1.25 * MEASURED_GOLDEN[1]


def test_float_budget():
    (la, ga), (ll, gl) = R.float_error("adjugate"), R.float_error("ldl")
    bl, bg = R.budgets()
    print(f"fp64 against longdouble: adjugate twin loss {la:.3e} grad {ga:.3e}; ldl twin loss {ll:.3e} grad {gl:.3e}")
    print(f"device budgets: loss {bl:.3e} of the scale, gradient {bg:.3e} + half an ulp of float32 at max |grad|")
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is no wider than fp64 here: the twin measures nothing"
    assert 0.0 < ll <= la and 0.0 < gl <= ga
    assert ll < 1e-13 and gl < 1e-14                # a few fp64 roundings, not a formula error
    assert bl == 16.0 * ll and bg == 16.0 * gl


@pytest.mark.parametrize("h,w,r", R.CASES)
def test_properties(h, w, r):
    noise = R.case(h, w, r, "noise")[2]
    assert (noise["loss"] >= 0.0).all() and (noise["closed"] >= 0.0).all()
    # the per-pixel sum and the per-window sum are the same number
    assert np.abs(noise["loss"] - noise["closed"]).max() <= 1e-12 * noise["scale"].max()
    const = R.case(h, w, r, "const")[2]
    assert np.array_equal(const["loss"], np.zeros(3)) and np.array_equal(const["grad"], np.zeros((3, h, w)))
    affine = R.case(h, w, r, "affine")[2]
    assert (np.abs(affine["loss"]) < 1e-6 * noise["loss"]).all(), (affine["loss"], noise["loss"])
    assert (R.case(h, w, r, "noise", True)[2]["loss"] >= 0.0).all()


def test_gradient_is_the_derivative():
    """2 L x / (h w) against central differences of the loss (a quadratic form: exact up to rounding)"""
    G, X, ref = R.case(7, 9, 3, "noise")
    X = np.array(X, np.float64)
    rng = np.random.default_rng(0)
    for _ in range(5):
        c, y, x = rng.integers(0, 3), rng.integers(0, 7), rng.integers(0, 9)
        d = np.zeros_like(X)
        d[c, y, x] = 1e-3
        num = (R.matting(G, X + d, 3)["loss"].sum() - R.matting(G, X - d, 3)["loss"].sum()) / 2e-3
        assert abs(num - ref["grad"][c, y, x]) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- import path
def test_compute_laplacian_handle_and_mask():
    from utils.MattingLaplacian import compute_laplacian, laplacian_loss_grad
    G = R.guide_of(8, 9, "noise", 1)
    M = compute_laplacian(G, win_rad=2)
    assert M.guide_u8.dtype == np.uint8 and M.win_rad == 2 and M.eps == 1e-7 and M.shape == (72, 72)
    assert compute_laplacian(G.astype(np.float64)).guide_u8.tobytes() == G.tobytes()
    with pytest.raises(NotImplementedError):
        compute_laplacian(G, mask=np.ones((8, 9), bool))
    import torch
    with pytest.raises(ValueError):
        laplacian_loss_grad(torch.zeros(3, 8, 9), M)


def test_compute_laplacian_reads_a_path(tmp_path):
    from PIL import Image
    from utils.MattingLaplacian import compute_laplacian
    G = R.guide_of(8, 9, "noise", 2)
    Image.fromarray(G).save(tmp_path / "g.png")
    assert compute_laplacian(str(tmp_path / "g.png")).guide_u8.tobytes() == G.tobytes()


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.vst_version() >= 117 and _lib.MATTING_MAX_RADIUS == 3
    for name in ("vst_matting_workspace_bytes", "vst_matting_loss_f32", "vst_matting_loss_u8"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    E_ARG, E_SHAPE = -1, -2
    n = C.c_size_t(0)
    # 24 bytes per tile: 16 x 16 (r = 1), 12 x 16 (r = 2), 10 x 12 (r = 3)
    for (h, w, r), tiles in (((1080, 1920, 1), 68 * 120), ((3, 3, 1), 1), ((8, 4100, 1), 257), ((70, 141, 2), 6 * 9),
                             ((7, 9, 3), 1), ((21, 25, 3), 3 * 3)):
        assert L.vst_matting_workspace_bytes(h, w, r, C.byref(n)) == 0 and n.value == 24 * tiles, (h, w, r, n.value)
    for h, w, r in ((2, 9, 1), (9, 2, 1), (4, 9, 2), (6, 9, 3), (9, 9, 0), (9, 9, 4), (9, 9, -1), (0, 9, 1), (8193, 8192, 1)):
        assert L.vst_matting_workspace_bytes(h, w, r, C.byref(n)) == E_SHAPE, (h, w, r)
    assert L.vst_matting_workspace_bytes(9, 9, 1, None) == E_ARG
    from vstnet_amd import matting
    assert matting.workspace_bytes(37, 53, 1) == 24 * 3 * 4
    with pytest.raises(_lib.VstError):
        matting.workspace_bytes(37, 53, 4)
    # the launching entry points refuse before they touch anything (p: a non-null address nothing dereferences)
    p = 4096
    for fn in (L.vst_matting_loss_f32, L.vst_matting_loss_u8):
        assert fn(p, p, 2, 9, 1, 1e-7, p, p, p, None) == E_SHAPE
        assert fn(p, p, 9, 9, 0, 1e-7, p, p, p, None) == E_SHAPE
        assert fn(p, p, 9, 9, 4, 1e-7, p, p, p, None) == E_SHAPE
        assert fn(p, p, 8193, 8192, 1, 1e-7, p, p, p, None) == E_SHAPE
        for eps in (0.0, -1e-7, float("inf"), float("nan")):
            assert fn(p, p, 9, 9, 1, eps, p, p, p, None) == E_ARG
        assert fn(None, p, 9, 9, 1, 1e-7, p, p, p, None) == E_ARG
        assert fn(p, None, 9, 9, 1, 1e-7, p, p, p, None) == E_ARG
        assert fn(p, p, 9, 9, 1, 1e-7, None, p, p, None) == E_ARG
        assert fn(p, p, 9, 9, 1, 1e-7, p, p, None, None) == E_ARG
        assert fn(p, p, 9, 9, 1, 1e-7, p + 4, p, p, None) == E_ARG          # loss3 off the 8-byte grid


def test_front_end_argument_checks():
    import torch
    from vstnet_amd.matting import MattingLoss, matting_loss
    g, x = torch.zeros((8, 9, 3), dtype=torch.uint8), torch.zeros((3, 8, 9))
    with pytest.raises(ValueError):
        matting_loss(g, x)                          # off the GPU: no fallback
    for r, eps in ((0, 1e-7), (4, 1e-7), (1.5, 1e-7), (1, 0.0), (1, float("inf"))):
        with pytest.raises((ValueError, RuntimeError)):
            MattingLoss((8, 9), r, eps, "cpu")


# ---------------------------------------------------------------------------------------------------------------- the files
def test_join_of_the_parts(tmp_path):
    from vstnet_amd import affinity as A
    whole = {i: (0.1 * i + 1e-9 / 3, 0.01 * i + 7e-5) for i in range(7)}
    A.write_csv(tmp_path / A.CSV_NAME, whole)
    bounds = [(0, 3), (3, 5), (5, 7)]
    parts = []
    for rank, (lo, hi) in enumerate(bounds):
        parts.append(A.write_csv(tmp_path / A.part_name(rank), {i: whole[i] for i in range(lo, hi)}))
    out = A.join_parts([parts[2], parts[0], parts[1]], tmp_path / "joined.csv", 7)
    assert open(out, "rb").read() == open(tmp_path / A.CSV_NAME, "rb").read()
    assert A.read_csv(out) == whole
    os.remove(parts[1])
    with pytest.raises(FileNotFoundError, match="affinity.part1.csv"):
        A.join_parts(parts, tmp_path / "again.csv", 7)
    with pytest.raises(ValueError, match="frame 3"):
        A.join_parts([parts[0], parts[2]], tmp_path / "again.csv", 7)
    with pytest.raises(ValueError, match="more than one"):
        A.join_parts([parts[0], parts[0]], tmp_path / "again.csv")
    assert A.frame_losses([1.0, 2.0, 3.0, 0.5, 0.25, 0.25]) == (6.0, 1.0) and A.frame_losses([1.0, 2.0, 3.0]) == (6.0,)
    line = A.summary(whole)
    assert "working size" in line and "full size" in line and "(frame 6)" in line
