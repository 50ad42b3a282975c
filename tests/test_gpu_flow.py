"""The optical-flow kernels on the card (csrc/flow.hip) against the fp64 numpy statement of tests/flow_ref.py.

Estimator: every element within one float32 ulp at max(|v|, 1) of the reference, and at most 1e-3 of the elements differing at
all.  The reference against its own longdouble form differs nowhere (test_flow_host.py), and the device takes the same fp64
operations in the same order without contraction, so the cap is the device's alone; the count is printed.  Consistency: equal to
the reference mask except on pixels whose two sides differ by less than 1e-9, which must be fewer than 1e-3 of the frame.  Masked
L1: bit-equal to the exact integer statement."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import flow_ref as R
import temporal_ref as T

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def pair(kind):
    """(ref, src) uint8 frames by name; made once"""
    if kind == "tiny":
        return R.make_pair(8, 8, 0.0, (0.5, 0.25))[:2]
    if kind in ("t1", "t2", "t3"):
        h, w, _, amp, shift = R.PAIRS[("t1", "t2", "t3").index(kind) + 1]
        return R.make_pair(h, w, amp, shift)[:2]
    if kind == "out_of_frame":                      # a shift that drives samples out of the frame
        return R.make_pair(61, 83, 1.0, (9.0, 6.0))[:2]
    if kind == "identical":
        a = R.to_u8(R.texture(37, 53, 3))
        return a, a.copy()
    if kind == "unrelated":                         # nothing to match: the clamp on delta acts
        return R.to_u8(R.texture(61, 83, 5)), R.to_u8(R.texture(61, 83, 6))
    raise KeyError(kind)


# (pair, levels, iters, radius): 8x8 with one level; 37x53 asking for more levels than exist; 61x83; 96x128 with 4 levels, which
# crosses the 32 x 32 tile's seams in both axes (3 x 4 tiles at level 0, 2 x 2 at level 1); radius 1 and 3, iterations 1 and 3
CASES = (("tiny", 1, 3, 3), ("tiny", 1, 1, 1), ("t1", 8, 3, 3), ("t2", 3, 3, 3), ("t2", 3, 1, 1), ("t2", 3, 3, 1), ("t2", 3, 1, 3),
         ("t3", 4, 3, 3), ("out_of_frame", 3, 3, 3), ("identical", 3, 3, 3), ("unrelated", 3, 3, 3))


@functools.lru_cache(maxsize=None)
def want_flow(kind, levels, iters, radius, swap=False):
    ref, src = pair(kind)
    if swap:
        ref, src = src, ref
    return R.estimate(ref, src, levels=levels, iters=iters, radius=radius)


@pytest.mark.parametrize("kind,levels,iters,radius", CASES)
def test_estimator_against_fp64(kind, levels, iters, radius):
    from vstnet_amd.flow import FlowEstimator, estimate_flow, level_count, workspace_bytes
    ref, src = pair(kind)
    h, w = ref.shape[:2]
    want = want_flow(kind, levels, iters, radius)
    got = estimate_flow(dev(ref), dev(src), levels=levels, iters=iters, radius=radius).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (2, h, w)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(1.0)))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    differing = int((got != want).sum())
    print(f"flow {kind} {h}x{w} levels {level_count(h, w, levels)} iters {iters} radius {radius}: {differing} of {got.size} "
          f"elements differ, max |err| {err.max():.3e}, max |flow| {np.abs(want).max():.3f}")
    assert (err <= ulp).all(), (kind, float((err / ulp).max()))
    assert differing <= 1e-3 * got.size, (kind, differing, got.size)
    if kind == "identical":
        assert not got.any()
    if kind == "unrelated":                         # the clamp acted: the field moved, and no further than the clamp allows
        assert np.abs(want).max() > 1.0 and np.abs(want).max() <= iters * (2 ** level_count(h, w, levels) - 1)
    # the object form, with a workspace of exactly the stated size: the same bits
    est = FlowEstimator((h, w), levels=levels, iters=iters, radius=radius)
    assert est.ws.numel() == workspace_bytes(h, w, levels)
    assert est(dev(ref), dev(src)).cpu().numpy().tobytes() == got.tobytes()


def test_two_runs_give_the_same_bits():
    from vstnet_amd.flow import estimate_flow
    ref, src = (dev(a) for a in pair("t3"))
    runs = [estimate_flow(ref, src, levels=4).cpu().numpy().tobytes() for _ in range(2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(estimate_flow(ref, src, levels=4).cpu().numpy().tobytes())
    assert runs[0] == runs[1] == runs[2]


@pytest.mark.parametrize("kind,levels", (("t1", 8), ("t3", 4), ("out_of_frame", 3), ("unrelated", 3)))
def test_consistency(kind, levels):
    from vstnet_amd.flow import FlowEstimator, consistency
    fwd, bwd = want_flow(kind, levels, 3, 3), want_flow(kind, levels, 3, 3, swap=True)
    want, margin = R.consistency(fwd, bwd)
    got = consistency(dev(fwd), dev(bwd)).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape and set(np.unique(got)) <= {0, 1}
    close = margin < 1e-9
    assert close.mean() < 1e-3 and ((got == want) | close).all(), (kind, int(close.sum()), int((got != want).sum()))
    print(f"consistency {kind}: valid share {want.mean():.3f}, {int(close.sum())} pixels within 1e-9 of the threshold, "
          f"{int((got != want).sum())} differ")
    if kind == "unrelated":
        assert want.mean() < 0.9                    # (a mask that rejects something)
    # the estimator's own chain: forward, backward, mask
    ref, src = (dev(a) for a in pair(kind))
    est = FlowEstimator(ref.shape[:2], levels=levels, mask=True)
    flow, valid = est.masked(ref, src)
    assert torch.equal(valid, consistency(flow, est.backward)) and torch.equal(flow, est(ref, src, out=torch.empty_like(flow)))


@pytest.mark.parametrize("h,w", ((8, 8), (37, 53), (128, 260)))
@pytest.mark.parametrize("with_flow", (True, False))
def test_masked_l1(h, w, with_flow):
    from vstnet_amd.temporal import TemporalLoss, temporal_loss, warp
    flow = T.make_flow(h, w, "real") if with_flow else None
    d_flow = None if flow is None else dev(flow)
    a, b = T.make_frame_u8(h, w, 0), T.make_frame_u8(h, w, 1)
    valid = (np.random.default_rng(h + w).random((h, w)) < 0.7).astype(np.uint8)
    valid[0, 0] = 255                               # any non-zero byte counts
    sums, want = R.l1_masked_u8(a, b, flow, valid)
    warped = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    got = temporal_loss(dev(a), dev(b), d_flow, warped_out=warped, valid=dev(valid))
    assert got.dtype == torch.float64 and got.shape == (4,) and got.cpu().numpy().tobytes() == want.tobytes(), (got, want, sums)
    assert torch.equal(warped, warp(dev(a), d_flow))
    assert TemporalLoss((h, w))(dev(a), dev(b), d_flow, valid=dev(valid)).cpu().numpy().tobytes() == want.tobytes()
    ones = temporal_loss(dev(a), dev(b), d_flow, valid=dev(np.ones((h, w), np.uint8))).cpu().numpy()
    assert ones[:3].tobytes() == temporal_loss(dev(a), dev(b), d_flow).cpu().numpy().tobytes() and ones[3] == 1.0
    none = temporal_loss(dev(a), dev(b), d_flow, valid=dev(np.zeros((h, w), np.uint8)), out=torch.ones(4, dtype=torch.float64, device="cuda"))
    assert none.cpu().numpy().tobytes() == np.zeros(4).tobytes()


def test_bad_arguments_leave_the_output_alone():
    from vstnet_amd import _lib
    from vstnet_amd.flow import estimate_flow, workspace_bytes
    L = _lib.lib()
    h, w = 16, 24
    a, b = dev(T.make_frame_u8(h, w, 0)), dev(T.make_frame_u8(h, w, 1))
    flow = torch.full((2, h, w), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.zeros(workspace_bytes(h, w, 5), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    E_ARG, E_SHAPE = -1, -2
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for hh, ww, lv, it, r in ((4, 24, 5, 3, 3), (16, 7, 5, 3, 3), (16, 24, 0, 3, 3), (16, 24, 9, 3, 3), (16, 24, 5, 0, 3),
                              (16, 24, 5, 17, 3), (16, 24, 5, 3, 0), (16, 24, 5, 3, 8)):
        assert L.vst_flow_lk_u8(p(a), p(b), hh, ww, lv, it, r, 1e-3, p(flow), p(ws), st) == E_SHAPE, (hh, ww, lv, it, r)
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        assert L.vst_flow_lk_u8(p(a), p(b), h, w, 5, 3, 3, lam, p(flow), p(ws), st) == E_ARG, lam
    assert L.vst_flow_lk_u8(p(a), p(b), h, w, 5, 3, 3, 1e-3, p(ws), p(ws), st) == E_ARG         # the flow inside the workspace
    assert L.vst_flow_lk_u8(p(a), None, h, w, 5, 3, 3, 1e-3, p(flow), p(ws), st) == E_ARG
    valid = torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
    assert L.vst_flow_consistency(p(flow), p(flow), 4, w, p(valid), st) == E_SHAPE
    assert L.vst_flow_consistency(p(flow), None, h, w, p(valid), st) == E_ARG
    loss = torch.full((4,), 5.0, dtype=torch.float64, device="cuda")
    assert L.vst_temporal_l1_masked_u8(p(a), p(b), None, p(valid), 4, w, p(loss), None, p(ws), st) == E_SHAPE
    assert L.vst_temporal_l1_masked_u8(p(a), p(b), None, None, h, w, p(loss), None, p(ws), st) == E_ARG
    assert L.vst_temporal_l1_masked_u8(p(a), p(b), None, p(valid), h, w, p(loss), p(a), p(ws), st) == E_ARG
    torch.cuda.synchronize()
    assert (flow == 7.0).all() and (valid == 9).all() and (loss == 5.0).all() and not ws.any()
    with pytest.raises(_lib.VstError):
        estimate_flow(a, b, radius=8)
    with pytest.raises(ValueError):
        estimate_flow(a.cpu(), b.cpu())
