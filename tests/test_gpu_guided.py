"""Guided upscale kernels (csrc/guided.hip) through the C ABI against the fp64 yardstick of tests/guided_ref.py.

The f32 form must lie within the float budget of guided_ref: 4 x max |guided_emul - guided_ref| over these very inputs
(tests/test_guided_host.py::test_float_budget measures it over the six shapes x two eps: 1.963e-7, so 7.85e-7).  The u8 form must lie within one count of
guided_ref's bytes and may differ only where the fp64 value * 255 lies within 255 x the budget of an integer - a condition on every
differing byte, not a share."""
import ctypes as C

import numpy as np
import pytest
import torch

import guided_ref as R

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_abi(G, P, S, r, eps, to_u8):
    """vst_guided_fit + vst_guided_apply_{u8,f32} on the current stream; returns a numpy array ([H,W,3] uint8 or [3,H,W] fp32)"""
    from vstnet_amd import _lib
    L = _lib.lib()
    h, w = G.shape[:2]
    H, W = S.shape[:2]
    g, p, s = (torch.from_numpy(np.array(a)).cuda() for a in (G, P, S))         # (copies: the shared inputs are read-only)
    n = C.c_size_t(0)
    _lib.check(L.vst_guided_workspace_bytes(h, w, r, C.byref(n)), "vst_guided_workspace_bytes")
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    coef = torch.empty((12, h, w), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.vst_guided_fit(_p(g), _p(p), h, w, r, eps, _p(coef), _p(ws), st), "vst_guided_fit")
    if to_u8:
        out = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
        _lib.check(L.vst_guided_apply_u8(_p(coef), h, w, _p(s), H, W, _p(out), st), "vst_guided_apply_u8")
    else:
        out = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(L.vst_guided_apply_f32(_p(coef), h, w, _p(s), H, W, _p(out), st), "vst_guided_apply_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_f32(got, ref, what):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: f32 max error {err:.3e} (budget {R.float_budget():.3e})")
    assert np.isfinite(got).all() and err <= R.float_budget(), (what, err, R.float_budget())


def check_u8(got, ref, what):
    """ref: the fp64 planes [3,H,W]"""
    want = np.moveaxis(R.quantise(ref), 0, 2)
    d = got.astype(int) - want.astype(int)
    v = np.moveaxis(ref, 0, 2) * 255.0
    near = np.abs(v - np.round(v)) <= 255.0 * R.float_budget()
    print(f"{what}: u8 bytes differing {int((d != 0).sum())} of {d.size}, max {int(np.abs(d).max())}")
    assert got.shape == want.shape and np.abs(d).max() <= 1, what
    assert near[d != 0].all(), (what, "a byte differs where the fp64 value is not next to an integer")


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("work_hw,full_hw,r", R.CASES)
def test_kernels_against_fp64(work_hw, full_hw, r, eps):
    G, P, S, ref = R.case(work_hw, full_hw, r, eps)
    what = f"{work_hw}->{full_hw} r={r} eps={eps}"
    check_f32(run_abi(G, P, S, r, eps, False), ref, what)
    check_u8(run_abi(G, P, S, r, eps, True), ref, what)


def test_affine_and_constant_on_the_card():
    """P = M I + c on a white-noise guide comes back as M S / 255 + c, a constant P as that constant: against the reference,
    within the budget (the reference has the properties to 1e-6: tests/test_guided_host.py)"""
    rng = np.random.default_rng(11)
    G = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    S = rng.integers(0, 256, (47, 61, 3), dtype=np.uint8)
    M = np.array([[0.9, 0.1, -0.2], [0.05, 0.7, 0.2], [-0.1, 0.15, 0.8]])
    c = np.array([0.05, -0.02, 0.1])
    P = (np.einsum("ck,khw->chw", M, np.moveaxis(G / 255.0, 2, 0)) + c[:, None, None]).astype(np.float32)
    for eps in (1e-9, 1e-4):
        check_f32(run_abi(G, P, S, 3, eps, False), R.guided_ref(G, P, S, 3, eps, False), f"affine eps={eps}")
    got = run_abi(G, P, S, 3, 1e-9, False)
    want = np.einsum("ck,hwk->chw", M, S / 255.0) + c[:, None, None]
    # (P itself is rounded to fp32 here: 6e-8 of input error on top of the budget and the reference's own 1e-6)
    assert np.abs(got - want).max() <= 1e-6 + R.float_budget() + 1e-7
    P = np.ascontiguousarray(np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32)[:, None, None], (3, 20, 24)))
    got = run_abi(G, P, S, 4, 1e-3, False)
    check_f32(got, R.guided_ref(G, P, S, 4, 1e-3, False), "constant")
    assert np.abs(got - np.array([0.25, 0.5, 0.75])[:, None, None]).max() <= R.float_budget()
    assert np.array_equal(run_abi(G, P, S, 4, 1e-3, True), np.broadcast_to(np.array([63, 127, 191], np.uint8), (47, 61, 3)))


def test_u8_epilogue_on_values_that_are_no_numbers():
    """the writer's epilogue at its edges, through vst_guided_apply_u8 itself: NaN -> 0, far above 1 -> 255, far below 0 -> 0"""
    from vstnet_amd import _lib
    (h, w), (H, W) = (5, 7), (11, 19)
    coef = torch.zeros((12, h, w), dtype=torch.float32, device="cuda")
    coef[9], coef[10], coef[11] = float("nan"), 1e30, -1e30      # (b alone: A = 0)
    src = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    out = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().vst_guided_apply_u8(_p(coef), h, w, _p(src), H, W, _p(out), st), "vst_guided_apply_u8")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to(np.array([0, 255, 0], np.uint8), (H, W, 3)))
    assert np.array_equal(R.quantise(np.array([np.nan, np.inf, -1e30])), [0, 255, 0])


def test_guided_upscale_object_equals_the_two_calls():
    from vstnet_amd.guided import GuidedUpscale, guided_apply, guided_fit
    (h, w), (H, W), r = R.CASES[3]
    G, P, S, ref = R.case((h, w), (H, W), r, 1e-4)
    g, p, s = (torch.from_numpy(np.array(a)).cuda() for a in (G, P, S))
    up = GuidedUpscale((h, w), (H, W), r, 1e-4, torch.device("cuda"))
    out = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    got = up(g[None], p[None], s, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (1, H, W, 3)
    coef = guided_fit(g, p, r, 1e-4)
    by_hand = guided_apply(coef, s)
    assert torch.equal(up.coef, coef) and torch.equal(got, by_hand)
    assert np.array_equal(by_hand[0].cpu().numpy(), run_abi(G, P, S, r, 1e-4, True))
    check_f32(guided_apply(coef, s, to_u8=False)[0].cpu().numpy(), ref, "guided_apply f32")
    again = up(g, p, s)                                              # the object's buffers serve the next frame
    assert torch.equal(again, by_hand)
    with pytest.raises(ValueError):
        up(g, p, s[:-1].contiguous())
    with pytest.raises(ValueError):
        GuidedUpscale((h, w), (H, W), 9, 1e-4, torch.device("cuda"))
    with pytest.raises(ValueError):
        GuidedUpscale((h, w), (h - 1, W), 4, 1e-4, torch.device("cuda"))
    with pytest.raises(ValueError):
        guided_fit(g.cpu(), p, r, 1e-4)
