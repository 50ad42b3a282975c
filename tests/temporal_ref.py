"""Numpy yardsticks of the temporal loss (csrc/temporal.hip, include/vstnet.h "Temporal loss"): the warp in fp32 in the documented
order of operations, the noise rules, the L1 mean in exact integers (uint8) and fp64 (float), the fake flow in fp64 from the
documented INTER_LINEAR and box-filter rules, and the pixels a warp test must exempt: those whose sampling coordinate lies so
close to a half that one fp32 rounding decides which neighbour is the nearest.

The warp yardstick equals torch's CPU grid_sample on the reference's grid pixel for pixel (tests/golden/temporal.npz, written by
tests/make_temporal_golden.py from the reference's own functions; test_temporal_host.py).  The fake flow has no such witness:
OpenCV is not available to this suite, so the yardstick states the documented rule and nothing checks it against cv2 itself."""
import numpy as np

F = np.float32

SIZES = ((8, 8), (12, 20), (37, 53), (100, 132))
FLOW_KINDS = ("real", "integer", "zero", "large")


# The near-tie band (near_tie: 1e-4 either side of a half, on two axes) covers 4e-4 of the coordinates, so a real-valued flow
# on 12 x 20 = 240 pixels has one such pixel in about one draw of ten - and one pixel of 240 is 4.2e-3 of the frame, above the
# 1e-3 the GPU test allows to be exempted.  At that size the test needs a draw with none; draw 0 has one, draw 1 has none.
DRAW = {(12, 20, "real"): 1}


def make_flow(h, w, kind, seed=None):
    """float32 [2,h,w]: real (a few pixels, fractional), integer (whole pixels), zero, large (beyond the frame both ways)"""
    seed = DRAW.get((h, w, kind), 0) if seed is None else seed
    rng = np.random.default_rng(1000 * seed + 10 * h + w + FLOW_KINDS.index(kind))
    if kind == "zero":
        return np.zeros((2, h, w), F)
    if kind == "integer":
        return rng.integers(-4, 5, (2, h, w)).astype(F)
    scale = 3.0 if kind == "real" else 2.5 * max(h, w)
    return (scale * rng.standard_normal((2, h, w))).astype(F)


def make_frame_f32(h, w, seed=0):
    return np.random.default_rng(77 + seed + 31 * h + w).random((3, h, w)).astype(F)


def make_frame_u8(h, w, seed=0):
    return np.random.default_rng(55 + seed + 31 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def axis_index(p, flo, n):
    """The source index along an axis of n pixels, every operation a rounded fp32 one, in the header's order."""
    p, flo = np.asarray(p, F), np.asarray(flo, F)
    v = p - flo
    t = (F(2.0) * v) / F(max(n - 1, 1)) - F(1.0)
    i = ((t + F(1.0)) * F(n) - F(1.0)) / F(2.0)
    assert i.dtype == F
    i = np.minimum(np.maximum(i, F(0.0)), F(n - 1))
    return np.rint(i).astype(np.int64)              # ties to even, as nearbyint


def source_index(flow, h, w):
    """(sy, sx): for every pixel, the pixel the warp reads"""
    if flow is None:
        return np.mgrid[0:h, 0:w]
    yy, xx = np.mgrid[0:h, 0:w]
    return axis_index(yy, flow[1], h), axis_index(xx, flow[0], w)


def warp_f32(x, flow, noise=None):
    """x float32 [3,h,w] -> warp(x, flow) [+ noise], float32"""
    h, w = x.shape[1:]
    sy, sx = source_index(flow, h, w)
    out = x[:, sy, sx]
    return out if noise is None else (out + noise.astype(F)).astype(F)


def warp_u8(x, flow, noise=None):
    """x uint8 [h,w,3] -> warp(x, flow), with noise: clamp(rint(float(v) + 255.0f * n), 0, 255) in fp32"""
    h, w = x.shape[:2]
    sy, sx = source_index(flow, h, w)
    out = x[sy, sx]
    if noise is None:
        return out
    t = out.astype(F) + F(255.0) * noise.astype(F).transpose(1, 2, 0)
    assert t.dtype == F
    return np.clip(np.rint(t), F(0.0), F(255.0)).astype(np.uint8)


def l1_u8(a, b, flow):
    """-> (per-channel integer sums as Python ints, the three values int_sum / (255.0 * h * w))"""
    h, w = a.shape[:2]
    d = np.abs(warp_u8(a, flow).astype(np.int64) - b.astype(np.int64))
    sums = [int(d[..., c].sum()) for c in range(3)]
    return sums, np.array([s / (255.0 * h * w) for s in sums], np.float64)


def l1_f32(a, b, flow):
    """-> the three means of |warp(a) - b| in fp64 (every difference of two floats is taken in fp64; math.fsum adds exactly)"""
    import math
    d = np.abs(warp_f32(a, flow).astype(np.float64) - b.astype(np.float64))
    return np.array([math.fsum(d[c].ravel()) / float(a.shape[1] * a.shape[2]) for c in range(3)], np.float64)


def near_tie(flow, h, w, eps=1e-4):
    """bool [h,w]: the pixels where the fp64 sampling coordinate of either axis (clamped as the warp clamps it) lies within eps
    of k + 0.5: there the fp32 roundings of the coordinate, not the rule, decide the neighbour."""
    out = np.zeros((h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for p, flo, n in ((xx, flow[0], w), (yy, flow[1], h)):
        v = p.astype(np.float64) - flo.astype(np.float64)
        i = ((2.0 * v / max(n - 1, 1) - 1.0 + 1.0) * n - 1.0) / 2.0
        i = np.clip(i, 0.0, n - 1.0)
        out |= np.abs(i - np.floor(i) - 0.5) <= eps
    return out


# ------------------------------------------------------------------------------------------------ the fake flow, fp64
def _linear_matrix(src, dst):
    """[dst, src]: the INTER_LINEAR weights, source coordinate (d + 0.5) * src / dst - 0.5, edges replicated"""
    m = np.zeros((dst, src), np.float64)
    for d in range(dst):
        s = (d + 0.5) * src / dst - 0.5
        i0 = int(np.floor(s))
        f = s - i0
        if i0 < 0:
            i0, f = 0, 0.0
        if i0 >= src - 1:
            i0, f = src - 1, 0.0
        m[d, i0] += 1.0 - f
        if f:
            m[d, i0 + 1] += f
    return m


def _reflect101(i, n):
    i = np.abs(i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def fake_flow(grid, shifts, h, w, ksize):
    """grid [gh,gw,2] (x first), shifts (x, y) -> float64 [2,h,w]: upsample, add the shifts, ksize x ksize box filter with anchor
    ksize // 2 (window x - ksize // 2 .. x - ksize // 2 + ksize - 1) under BORDER_REFLECT_101, normalised."""
    g = np.asarray(grid, np.float64)
    gh, gw = g.shape[:2]
    assert min(h, w) >= ksize >= 1 and gh >= 1 and gw >= 1
    up = np.einsum("yg,ghc,xh->cyx", _linear_matrix(gh, h), g, _linear_matrix(gw, w))
    up[0] += float(shifts[0])
    up[1] += float(shifts[1])
    taps = np.arange(ksize) - ksize // 2
    rows = _reflect101(np.arange(h)[:, None] + taps[None, :], h)        # [h, k]
    cols = _reflect101(np.arange(w)[:, None] + taps[None, :], w)        # [w, k]
    tmp = up[:, rows, :].sum(axis=2)                                    # [2, h, w]: the vertical taps
    out = tmp[:, :, cols].sum(axis=3)                                   # the horizontal taps
    return out / float(ksize * ksize)


FLOW_CASES = ((16, 20, 4, 6), (37, 53, 10, 7), (200, 300, 100, 100))


def flow_draws(h, w, cell, seed=0):
    rng = np.random.default_rng(900 + seed + h + w)
    return rng.normal(0.0, 8.0, (h // cell, w // cell, 2)), (int(rng.integers(-10, 11)), int(rng.integers(-10, 11)))
