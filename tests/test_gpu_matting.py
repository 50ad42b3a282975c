"""The affinity-loss kernels (csrc/matting.hip) through the C ABI against the fp64 yardstick of tests/matting_ref.py.

Budgets (matting_ref.budgets(); tests/test_matting_host.py::test_float_budget measures and prints them): 16 x the largest
deviation of the fp64 yardstick from its longdouble twin over CASES x the three forms of x used here - for the loss, relative to
the uncancelled magnitude sum_k n var_k(x) / (h w): MEASURED_LOSS; for the gradient, absolute: MEASURED_GRAD, plus half an ulp of
float32 at max |grad| because the device stores the gradient as float32.
MEASURED_LOSS = 5.33e-15 (budget 8.54e-14), MEASURED_GRAD = 3.28e-17 (budget 5.25e-16 + half an ulp).
(Against the issue's adjugate twin the figures are 2.07e-7 and 1.85e-10, all of it the adjugate's own loss on the step case's
rank-one windows; the budgets take the smaller figure.)
Measured on an MI355X: the loss within 1.29e-15 of the scale on every case and form; the float32 gradient within half an ulp at
max |grad| (2.31e-10 at 37x53, budget 2.33e-10); the affine cases' gradients within 8.8e-16; against the reference's own
matrix through utils.MattingLaplacian 4.6e-8 relative on the loss and 9.9e-8 of the largest entry on the gradient."""
import ctypes as C

import numpy as np
import pytest
import torch

import matting_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_SHAPE = -1, -2


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def run_abi(G, X, r, eps=R.EPS, grad=True):
    """vst_matting_loss_{f32,u8} on the current stream -> (loss float64 [3], grad float32 [3,h,w] or None).  The outputs are
    pre-filled with NaN.  Without the gradient the buffer is still made, as a guard: it is not passed and must stay as it was."""
    from vstnet_amd import _lib
    L = _lib.lib()
    h, w = G.shape[:2]
    g, x = torch.from_numpy(np.array(G)).cuda(), torch.from_numpy(np.array(X)).cuda()
    n = C.c_size_t(0)
    _lib.check(L.vst_matting_workspace_bytes(h, w, r, C.byref(n)), "vst_matting_workspace_bytes")
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    loss = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    fn = L.vst_matting_loss_u8 if X.dtype == np.uint8 else L.vst_matting_loss_f32
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(fn(_p(g), _p(x), h, w, r, eps, _p(loss), _p(out) if grad else None, _p(ws), st), "vst_matting_loss")
    torch.cuda.synchronize()
    if not grad:
        assert torch.isnan(out).all(), "the gradient buffer was written though no pointer to it was passed"
    return loss.cpu().numpy(), (out.cpu().numpy() if grad else None)


def check(got_loss, got_grad, ref, what):
    bl, bg = R.budgets(float(np.abs(ref["grad"]).max()))
    el = float(np.abs((got_loss - ref["loss"]) / np.where(ref["scale"] > 0, ref["scale"], 1.0)).max())
    print(f"{what}: loss deviation {el:.3e} of the scale (budget {bl:.3e})")
    assert np.isfinite(got_loss).all() and el <= bl, (what, el, bl)
    if got_grad is not None:
        eg = float(np.abs(got_grad.astype(np.float64) - ref["grad"]).max())
        print(f"{what}: gradient deviation {eg:.3e} (budget {bg:.3e})")
        assert np.isfinite(got_grad).all() and eg <= bg, (what, eg, bg)


@pytest.mark.parametrize("grad", (True, False))
@pytest.mark.parametrize("u8", (False, True))
@pytest.mark.parametrize("h,w,r", R.CASES)
def test_kernels_against_fp64(h, w, r, u8, grad):
    G, X, ref = R.case(h, w, r, "noise", u8)
    loss, g = run_abi(G, X, r, grad=grad)
    check(loss, g, ref, f"{h}x{w} r={r} {'u8' if u8 else 'f32'}")


@pytest.mark.parametrize("h,w,r", [(37, 53, 1), (70, 141, 2), (7, 9, 3)])
def test_same_call_twice_same_bits(h, w, r):
    G, X, _ = R.case(h, w, r, "noise", False)
    a, b = run_abi(G, X, r), run_abi(G, X, r)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = run_abi(G, X, r, grad=False)                        # the gradient pointer does not change the loss
    assert c[0].tobytes() == a[0].tobytes()


@pytest.mark.parametrize("h,w,r", R.CASES)
def test_affine_and_constant_on_the_card(h, w, r):
    G, X, ref = R.case(h, w, r, "affine", False)
    check(*run_abi(G, X, r), ref, f"{h}x{w} r={r} affine")
    G, X, ref = R.case(h, w, r, "const", False)
    loss, g = run_abi(G, X, r)
    assert np.array_equal(loss, np.zeros(3)) and np.array_equal(g, np.zeros((3, h, w), np.float32))
    loss, g = run_abi(G, R.as_u8(np.array(X)), r)
    assert np.array_equal(loss, np.zeros(3)) and np.array_equal(g, np.zeros((3, h, w), np.float32))


def test_rejections_before_launch():
    from vstnet_amd import _lib
    L = _lib.lib()
    G, X, _ = R.case(37, 53, 1, "noise", False)
    g, x = torch.from_numpy(np.array(G)).cuda(), torch.from_numpy(np.array(X)).cuda()
    xu = torch.from_numpy(R.as_u8(np.array(X))).cuda()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    loss = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((3, 37, 53), -7.0, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn, xx in ((L.vst_matting_loss_f32, x), (L.vst_matting_loss_u8, xu)):
        assert fn(_p(g), _p(xx), 2, 53, 1, 1e-7, _p(loss), _p(out), _p(ws), st) == E_SHAPE           # h < 2 r + 1
        assert fn(_p(g), _p(xx), 6, 53, 3, 1e-7, _p(loss), _p(out), _p(ws), st) == E_SHAPE
        assert fn(_p(g), _p(xx), 37, 53, 0, 1e-7, _p(loss), _p(out), _p(ws), st) == E_SHAPE
        assert fn(_p(g), _p(xx), 37, 53, 4, 1e-7, _p(loss), _p(out), _p(ws), st) == E_SHAPE
        assert fn(_p(g), _p(xx), 37, 53, 1, 0.0, _p(loss), _p(out), _p(ws), st) == E_ARG
        assert fn(_p(g), _p(xx), 37, 53, 1, float("nan"), _p(loss), _p(out), _p(ws), st) == E_ARG
        assert fn(_p(g), _p(xx), 37, 53, 1, 1e-7, None, _p(out), _p(ws), st) == E_ARG
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all()) and bool((out == -7.0).all())


def test_python_front_end():
    from vstnet_amd.matting import MattingLoss, matting_loss, workspace_bytes
    h, w, r = 37, 53, 1
    G, X, ref = R.case(h, w, r, "noise", False)
    g, x = torch.from_numpy(np.array(G)).cuda(), torch.from_numpy(np.array(X)).cuda()
    loss, grad = matting_loss(g[None], x[None], r, R.EPS, grad=True)
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (3,) and loss.is_cuda
    assert grad.dtype == torch.float32 and tuple(grad.shape) == (3, h, w)
    want = run_abi(G, X, r)
    assert loss.cpu().numpy().tobytes() == want[0].tobytes() and grad.cpu().numpy().tobytes() == want[1].tobytes()
    only = matting_loss(g, x, r, R.EPS)
    assert torch.is_tensor(only) and torch.equal(only, loss)
    xu = torch.from_numpy(R.as_u8(np.array(X))).cuda()
    check(matting_loss(g, xu).cpu().numpy(), None, R.case(h, w, r, "noise", True)[2], "front end u8")
    m = MattingLoss((h, w), r, R.EPS, torch.device("cuda"), grad=True)
    l2, g2 = m(g, x)
    assert l2.data_ptr() == m.loss.data_ptr() and torch.equal(l2, loss) and torch.equal(g2, grad)
    assert m.ws.numel() == workspace_bytes(h, w, r)
    with pytest.raises(ValueError):
        matting_loss(g.cpu(), x)
    with pytest.raises(ValueError):
        matting_loss(g, x.cpu())
    with pytest.raises(ValueError):
        m(g[:-1].contiguous(), x)
    from vstnet_amd._lib import VstError
    with pytest.raises(VstError):
        matting_loss(g, x, 4)


def test_reference_import_path_against_the_reference():
    """utils.MattingLaplacian with the reference's call sequence against what the reference's own matrix gives
    (tests/golden/matting.npz): within the host test's tolerance (4 x the largest deviation of the yardstick from the golden)
    plus the device budget."""
    import os
    from utils.MattingLaplacian import compute_laplacian, laplacian_loss_grad
    from test_matting_host import golden_tolerance
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matting.npz"))
    tol_l, tol_g = golden_tolerance()
    for name in ("noise", "ramp"):
        for r in (1, 2):
            G, X = gold[f"{name}_guide"], gold[f"{name}_x"]
            M = compute_laplacian(G, eps=float(gold["eps"]), win_rad=r)
            image = torch.from_numpy(X).cuda()
            loss, grad = laplacian_loss_grad(image, M)
            assert tuple(loss.shape) == (1, 1) and loss.dtype == image.dtype and loss.device == image.device
            assert tuple(grad.shape) == tuple(X.shape) and grad.dtype == image.dtype and grad.device == image.device
            want_l, want_g = float(gold[f"{name}_r{r}_loss"]), gold[f"{name}_r{r}_grad2"]
            bl, bg = R.budgets(float(np.abs(want_g).max()))
            bl *= float(R.matting(G, X, r, float(gold["eps"]))["scale"].sum()) / want_l       # (from the scale to the loss)
            el = abs(float(loss) - want_l) / want_l
            eg = float(np.abs(grad.cpu().numpy().astype(np.float64) - want_g).max() / np.abs(want_g).max())
            print(f"{name} r={r}: loss {el:.3e} relative, gradient {eg:.3e} of its largest entry")
            # (the [1,1] loss is in image.dtype, float32 here: half an ulp of float32 on top)
            assert el <= tol_l + bl + 2.0 ** -24
            assert eg <= tol_g + bg / np.abs(want_g).max()
    with pytest.raises(ValueError):
        laplacian_loss_grad(torch.from_numpy(gold["noise_x"]), compute_laplacian(gold["noise_guide"]))
