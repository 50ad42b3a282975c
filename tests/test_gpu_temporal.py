"""The temporal-loss kernels on the card (csrc/temporal.hip) against the numpy yardsticks of tests/temporal_ref.py.

Warp: equal to the fp32 restatement at every pixel outside near_tie - the pixels whose fp64 sampling coordinate lies within 1e-4 of
a half, where one fp32 rounding of the coordinate and not the rule decides the neighbour; the test asserts that these are at most
1e-3 of the frame and prints how many it exempted.  (The device does the same fp32 operations in the same order without
contraction, so it is expected to agree there too; the exemption is the issue's, and the count of actual differences is printed.)
L1: the uint8 loss is bit-equal to int_sum / (255.0 h w); the float loss lies within h w 2^-53 relative of the exactly added
fp64 yardstick - h w fp64 additions of non-negative terms, half an ulp each.  Fake flow: within half an fp32 ulp at max |flow|,
plus 1e-12, of the fp64 yardstick - the device's fp64 sums differ from numpy's by rounding order only, 1e-12 covers that, the
half ulp is the one rounding to float32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import temporal_ref as R

pytestmark = pytest.mark.gpu

L1_SIZES = ((8, 8), (37, 53), (128, 260))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def noise_of(h, w):
    n = (0.05 * np.random.default_rng(5 + h + w).standard_normal((3, h, w))).astype(np.float32)
    n[:, 0, 0] = (3.0, -3.0, 0.5 / 255.0)           # both saturations and a tie of the uint8 rule
    return n


@pytest.mark.parametrize("h,w", R.SIZES)
@pytest.mark.parametrize("kind", R.FLOW_KINDS)
def test_warp(h, w, kind):
    from vstnet_amd.temporal import warp
    flow = R.make_flow(h, w, kind)
    tie = R.near_tie(flow, h, w)
    share = float(tie.mean())
    assert share <= 1e-3, (h, w, kind, share)
    if kind in ("integer", "zero"):
        assert share == 0.0
    differing = 0
    xf, xu = R.make_frame_f32(h, w), R.make_frame_u8(h, w)
    for noise in (None, noise_of(h, w)):
        d_noise = None if noise is None else dev(noise)
        got_f = warp(dev(xf), dev(flow), d_noise).cpu().numpy()
        got_u = warp(dev(xu), dev(flow), d_noise).cpu().numpy()
        want_f, want_u = R.warp_f32(xf, flow, noise), R.warp_u8(xu, flow, noise)
        assert got_f.dtype == np.float32 and got_u.dtype == np.uint8
        ok_f = (got_f.view(np.uint32) == want_f.view(np.uint32)).all(axis=0)
        ok_u = (got_u == want_u).all(axis=2)
        assert (ok_f | tie).all() and (ok_u | tie).all(), (h, w, kind, noise is not None, int((~ok_f).sum()), int((~ok_u).sum()))
        differing += int((~ok_f).sum()) + int((~ok_u).sum())
        if kind == "zero" and noise is None:        # the identity, and the null flow is the same thing
            assert np.array_equal(got_f, xf) and np.array_equal(got_u, xu)
            assert np.array_equal(warp(dev(xu), None).cpu().numpy(), xu)
    print(f"warp {h}x{w} {kind}: {int(tie.sum())} of {h * w} pixels exempted as near ties ({share:.2e}); "
          f"{differing} values differ there")


@pytest.mark.parametrize("h,w", L1_SIZES)
@pytest.mark.parametrize("with_flow", (True, False))
def test_l1(h, w, with_flow):
    from vstnet_amd.temporal import TemporalLoss, temporal_loss, warp, workspace_bytes
    flow = R.make_flow(h, w, "real") if with_flow else None
    d_flow = None if flow is None else dev(flow)
    assert workspace_bytes(h, w) == 24 * ((h * w + 2047) // 2048)
    # uint8: exact
    a, b = R.make_frame_u8(h, w, 0), R.make_frame_u8(h, w, 1)
    sums, want = R.l1_u8(a, b, flow)
    warped = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    got = temporal_loss(dev(a), dev(b), d_flow, warped_out=warped)
    assert got.dtype == torch.float64 and got.cpu().numpy().tobytes() == want.tobytes(), (got, want, sums)
    assert torch.equal(warped, warp(dev(a), d_flow))
    again = TemporalLoss((h, w))(dev(a), dev(b), d_flow)
    assert again.cpu().numpy().tobytes() == want.tobytes()
    # float32: h w fp64 additions
    x, y = R.make_frame_f32(h, w, 0), R.make_frame_f32(h, w, 1)
    want_f = R.l1_f32(x, y, flow)
    warped_f = torch.zeros((3, h, w), dtype=torch.float32, device="cuda")
    got_f = temporal_loss(dev(x), dev(y), d_flow, warped_out=warped_f).cpu().numpy()
    rel = np.abs(got_f - want_f) / want_f
    print(f"l1 {h}x{w} flow={with_flow}: float loss {rel.max():.2e} relative off the fp64 yardstick (bound {h * w * 2.0 ** -53:.2e})")
    assert (rel <= h * w * 2.0 ** -53).all()
    assert torch.equal(warped_f, warp(dev(x), d_flow))
    # two runs, the second on another stream with its own buffers: the same bits
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        second = temporal_loss(dev(x), dev(y), d_flow).cpu().numpy()
    st.synchronize()
    assert second.tobytes() == got_f.tobytes()
    # a pair that agrees under the warp costs nothing
    assert (temporal_loss(dev(a), warp(dev(a), d_flow), d_flow).cpu().numpy() == 0.0).all()


@pytest.mark.parametrize("h,w,cell,ksize", R.FLOW_CASES)
def test_fake_flow(h, w, cell, ksize):
    from vstnet_amd.temporal import fake_flow, fake_flow_from
    grid, shifts = R.flow_draws(h, w, cell)
    want = R.fake_flow(grid, shifts, h, w, ksize)
    got = fake_flow_from(grid, shifts, (h, w), ksize).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (2, h, w)
    tol = 0.5 * float(np.spacing(np.float32(np.abs(want).max()))) + 1e-12
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"fake flow {h}x{w} cell {cell} ksize {ksize}: max |flow| {np.abs(want).max():.3f}, error {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    # a float32 grid is read as its float64 values, and the front end draws what draw_fake_flow draws
    got32 = fake_flow_from(grid.astype(np.float32), shifts, (h, w), ksize).cpu().numpy()
    assert np.abs(got32 - R.fake_flow(grid.astype(np.float32), shifts, h, w, ksize)).max() <= tol
    from vstnet_amd.temporal import draw_fake_flow
    g2, s2 = draw_fake_flow((h, w), np.random.default_rng(4), 8, 10, cell)
    f2 = fake_flow((h, w), np.random.default_rng(4), 8, 10, cell, ksize).cpu().numpy()
    assert np.abs(f2 - R.fake_flow(g2, s2, h, w, ksize)).max() <= 0.5 * float(np.spacing(np.float32(np.abs(f2).max()))) + 1e-12
    still = fake_flow((h, w), np.random.default_rng(4), 0, 10).cpu().numpy()        # motion_level 0: the two shifts alone
    assert still.shape == (2, h, w) and (still[0] == still[0, 0, 0]).all() and (still[1] == still[1, 0, 0]).all()


def test_fake_flow_shape_errors_launch_nothing():
    from vstnet_amd import _lib
    from vstnet_amd.temporal import fake_flow_from
    L = _lib.lib()
    flow = torch.full((2, 16, 20), 7.0, dtype=torch.float32, device="cuda")
    grid = torch.zeros((4, 5, 2), dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for gh, gw, k in ((0, 5, 6), (4, 0, 6), (4, 5, 17), (4, 5, 0), (1025, 5, 6)):
        assert L.vst_fake_flow(ptr(grid), gh, gw, 0.0, 0.0, k, ptr(flow), 16, 20, ptr(ws), None) == -2
    torch.cuda.synchronize()
    assert (flow == 7.0).all()                      # nothing ran
    with pytest.raises(_lib.VstError):
        fake_flow_from(np.zeros((4, 5, 2)), (0, 0), (16, 20), 17)


def test_import_path_on_the_card():
    """utils.TemporalLoss: the reference's call sequence; what forward returns is the library's loss and warp, in the input's
    dtype; GenerateFakeData without noise and without motion is the identity."""
    import random
    from utils.TemporalLoss import TemporalLoss, warp
    from vstnet_amd import temporal
    h, w = 37, 53
    x = dev(np.stack([R.make_frame_f32(h, w, 0), R.make_frame_f32(h, w, 2)]))
    y = dev(np.stack([R.make_frame_f32(h, w, 1), R.make_frame_f32(h, w, 3)]))
    flow = dev(np.stack([R.make_flow(h, w, "real"), R.make_flow(h, w, "integer")]))
    loss_fn = TemporalLoss()
    loss, warped = loss_fn(x, y, flow)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and warped.shape == x.shape
    want = np.mean([R.l1_f32(x[b].cpu().numpy(), y[b].cpu().numpy(), flow[b].cpu().numpy()).mean() for b in range(2)])
    assert abs(float(loss) - want) <= 2.0 ** -23 * want
    assert torch.equal(warped, warp(x, flow)) and torch.equal(warped[1], temporal.warp(x[1], flow[1]))
    half, _ = loss_fn(x.half(), y.half(), flow)
    assert half.dtype == torch.float16
    loss_fn.cell, loss_fn.ksize = 10, 7
    random.seed(3)
    np.random.seed(3)
    second, f = loss_fn.GenerateFakeData(x)
    assert second.shape == x.shape and f.shape == (2, 2, h, w) and torch.equal(f[0], f[1])
    assert float((second - warp(x, f)).abs().max()) < 0.02 and float((second - warp(x, f)).abs().max()) > 0.0    # the noise
    plain = TemporalLoss(data_sigma=False, data_w=False)
    same, none = plain.GenerateFakeData(x)
    assert none is None and torch.equal(same, x)
    zero, first = plain(x, x, None)
    assert float(zero) == 0.0 and first is x


def test_synthetic_clip():
    from vstnet_amd.temporal import synthetic_clip, temporal_loss, mean3
    still = R.make_frame_u8(64, 96)
    frames, flows, loss_in = synthetic_clip(still, 4, seed=5, cell=16, ksize=16)
    assert frames.shape == (4, 64, 96, 3) and frames.dtype == torch.uint8 and flows.shape == (4, 2, 64, 96)
    assert loss_in.shape == (4,) and loss_in.dtype == torch.float64
    assert np.array_equal(frames[0].cpu().numpy(), still) and not flows[0].any()
    li = loss_in.cpu().numpy()
    assert np.isnan(li[0]) and (li[1:] > 0).all() and (li[1:] < 0.01).all()         # the noise alone: a few levels of 255 at most
    for t in range(1, 4):
        assert mean3(temporal_loss(frames[t - 1], frames[t], flows[t]).cpu().numpy()) == li[t]
    again = synthetic_clip(still, 4, seed=5, cell=16, ksize=16)
    assert torch.equal(again[0], frames) and torch.equal(again[1], flows)
    other = synthetic_clip(still, 4, seed=6, cell=16, ksize=16)
    assert not torch.equal(other[0], frames)
