"""Numpy yardsticks of the optical flow (csrc/flow.hip, include/vstnet.h "Optical flow"): the coarse-to-fine warping Lucas-Kanade
estimator with the number format as a parameter (float64 is the statement the device is held to; longdouble shows how far float64
itself is from the formulas; float32 shows what a cheaper device format would cost), the forward-backward consistency rule with
the margin of every pixel to its threshold, the masked L1 mean in exact integers, and the generators of the test pairs: a seeded
multi-scale texture and a smooth flow under which it is resampled.

Every sum is taken in the order the header states: a window's columns first, in increasing order, then its rows."""
import numpy as np

from temporal_ref import warp_u8

# (h, w, levels, amp, shift): the pairs of the issue's table; the first four carry the accuracy condition
PAIRS = ((40, 56, 3, 0.0, (1.0, 0.0)), (37, 53, 8, 0.5, (0.4, -0.3)), (61, 83, 3, 1.0, (2.5, -1.5)), (96, 128, 4, 1.5, (4.0, -2.0)),
         (128, 160, 5, 2.0, (9.0, 6.0)))
BINOMIAL = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def level_shapes(h, w, levels):
    """The pyramid's shapes: a level is added while fewer than `levels` exist and the new level's shorter edge is at least 8."""
    out = [(int(h), int(w))]
    while len(out) < levels:
        nh, nw = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if min(nh, nw) < 8:
            break
        out.append((nh, nw))
    return out


def _taps(n, r):
    """[n, 2r+1]: the window's coordinates along an axis of n pixels, clamped to the frame"""
    return np.clip(np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :], 0, n - 1)


def window(a, r, weights=None):
    """The (2r+1)^2 window sum of a [h,w] plane with clamped coordinates: columns first, then rows, each in increasing order."""
    h, w = a.shape
    xs, ys = _taps(w, r), _taps(h, r)
    t = np.zeros_like(a)
    for k in range(2 * r + 1):
        t = t + (a[:, xs[:, k]] if weights is None else a.dtype.type(weights[k]) * a[:, xs[:, k]])
    s = np.zeros_like(a)
    for k in range(2 * r + 1):
        s = s + (t[ys[:, k], :] if weights is None else a.dtype.type(weights[k]) * t[ys[:, k], :])
    return s


def binomial5(a):
    return window(a, 2, BINOMIAL)


def bilinear(a, y, x):
    """bilinear(A; y, x) of the header: coordinates clamped to the frame, x1 = min(x0 + 1, n - 1)."""
    h, w = a.shape
    t = a.dtype.type
    x = np.clip(x, t(0), t(w - 1))
    y = np.clip(y, t(0), t(h - 1))
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = x - x0.astype(a.dtype), y - y0.astype(a.dtype)
    top = (t(1) - fx) * a[y0, x0] + fx * a[y0, x1]
    bot = (t(1) - fx) * a[y1, x0] + fx * a[y1, x1]
    return (t(1) - fy) * top + fy * bot


def grey(u8, dtype):
    t = np.dtype(dtype).type
    f = u8.astype(dtype)
    return (t(0.299) * f[..., 0] + t(0.587) * f[..., 1] + t(0.114) * f[..., 2]) / t(255)


def inside_weight(c, n):
    t = c.dtype.type
    o = np.maximum(np.maximum(-c, c - t(n - 1)), t(0))
    return np.minimum(np.maximum(t(1) - o, t(0)), t(1))


def estimate(ref_u8, src_u8, levels=5, iters=3, radius=3, lam=1e-3, dtype=np.float64, raw=False):
    """The estimator of the header -> flow float32 [2,h,w] (raw: d_0 = -flow in `dtype`, before the rounding)."""
    dtype = np.dtype(dtype)
    t = dtype.type
    h, w = ref_u8.shape[:2]
    R, S = [grey(ref_u8, dtype)], [grey(src_u8, dtype)]
    for nh, nw in level_shapes(h, w, levels)[1:]:
        R.append(binomial5(R[-1])[::2, ::2])
        S.append(binomial5(S[-1])[::2, ::2])
        assert R[-1].shape == (nh, nw)
    dx = dy = None
    for l in range(len(R) - 1, -1, -1):
        r_l, s_l = R[l], S[l]
        lh, lw = r_l.shape
        yy, xx = (g.astype(dtype) for g in np.mgrid[0:lh, 0:lw])
        if dx is None:
            dx, dy = np.zeros((lh, lw), dtype), np.zeros((lh, lw), dtype)
        else:
            dx, dy = t(2) * bilinear(dx, t(0.5) * yy, t(0.5) * xx), t(2) * bilinear(dy, t(0.5) * yy, t(0.5) * xx)
        xi, yi = np.arange(lw), np.arange(lh)
        rx = (r_l[:, np.minimum(xi + 1, lw - 1)] - r_l[:, np.maximum(xi - 1, 0)]) / t(2)
        ry = (r_l[np.minimum(yi + 1, lh - 1), :] - r_l[np.maximum(yi - 1, 0), :]) / t(2)
        a11, a12, a22 = window(rx * rx, radius) + t(lam), window(rx * ry, radius), window(ry * ry, radius) + t(lam)
        det = a11 * a22 - a12 * a12
        for _ in range(iters):
            sx, sy = xx + dx, yy + dy
            e = (bilinear(s_l, sy, sx) - r_l) * inside_weight(sy, lh) * inside_weight(sx, lw)
            b1, b2 = window(rx * e, radius), window(ry * e, radius)
            ux = np.clip(-((a22 * b1 - a12 * b2) / det), t(-1), t(1))
            uy = np.clip(-((a11 * b2 - a12 * b1) / det), t(-1), t(1))
            dx, dy = binomial5(dx + ux), binomial5(dy + uy)
    d = np.stack([dx, dy])
    return d if raw else (-d).astype(np.float32)


def consistency(fwd, bwd):
    """-> (valid uint8 [h,w], margin float64 [h,w]): margin = |rhs - lhs| of the rule where q is inside the frame (inf outside,
    where the rule is not consulted)"""
    f, b = fwd.astype(np.float64), bwd.astype(np.float64)
    h, w = f.shape[1:]
    yy, xx = (g.astype(np.float64) for g in np.mgrid[0:h, 0:w])
    qx, qy = xx - f[0], yy - f[1]
    inside = (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
    bx, by = bilinear(b[0], qy, qx), bilinear(b[1], qy, qx)
    sx, sy = f[0] + bx, f[1] + by
    lhs = sx * sx + sy * sy
    rhs = 0.01 * ((f[0] * f[0] + f[1] * f[1]) + (bx * bx + by * by)) + 0.5
    return (inside & (lhs <= rhs)).astype(np.uint8), np.where(inside, np.abs(rhs - lhs), np.inf)


def l1_masked_u8(a, b, flow, valid):
    """-> (the three integer sums and the count as Python ints, the four values of vst_temporal_l1_masked_u8)"""
    h, w = a.shape[:2]
    m = valid != 0
    d = np.abs(warp_u8(a, flow).astype(np.int64) - b.astype(np.int64))
    sums, count = [int(d[..., c][m].sum()) for c in range(3)], int(m.sum())
    vals = [s / (255.0 * count) for s in sums] + [count / float(h * w)] if count else [0.0] * 4
    return sums + [count], np.array(vals, np.float64)


# ------------------------------------------------------------------------------------------------ the test pairs
def _upsample(a, h, w):
    """a coarse [gh,gw] plane stretched bilinearly over [h,w], corner to corner"""
    gh, gw = a.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return bilinear(a, yy * ((gh - 1) / max(h - 1, 1)), xx * ((gw - 1) / max(w - 1, 1)))


def texture(h, w, seed=0):
    """float64 [h,w,3] in [0,1]: five scales of binomial-blurred Gaussian noise (scale s drawn on a grid 2^s times coarser),
    weights 1.5^s, normalised per channel."""
    rng = np.random.default_rng(4100 + 131 * seed + 7 * h + w)
    out = np.zeros((h, w, 3))
    for c in range(3):
        acc = np.zeros((h, w))
        for s in range(5):
            gh, gw = max(-(-h // 2 ** s), 2), max(-(-w // 2 ** s), 2)
            acc += 1.5 ** s * binomial5(_upsample(binomial5(rng.standard_normal((gh, gw))), h, w))
        out[..., c] = (acc - acc.min()) / (acc.max() - acc.min())
    return out


def smooth_flow(h, w, amp, shift, seed=0):
    """float64 [2,h,w]: a coarse Gaussian grid (one node per 16 pixels) stretched bilinearly, twice binomial-blurred, times amp,
    plus the shift (x, y)"""
    rng = np.random.default_rng(5200 + 17 * seed + 3 * h + w)
    out = np.zeros((2, h, w))
    for c in range(2):
        g = rng.standard_normal((h // 16 + 2, w // 16 + 2))
        out[c] = amp * binomial5(binomial5(_upsample(g, h, w))) + shift[c]
    return out


def to_u8(f):
    return np.clip(np.rint(255.0 * f), 0, 255).astype(np.uint8)


def make_pair(h, w, amp, shift, seed=0):
    """-> (ref uint8 [h,w,3], src uint8 [h,w,3], flow float64 [2,h,w]) with ref = bilinear(src texture; p - flow)"""
    tex, flow = texture(h, w, seed), smooth_flow(h, w, amp, shift, seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ref = np.stack([bilinear(np.ascontiguousarray(tex[..., c]), yy - flow[1], xx - flow[0]) for c in range(3)], axis=-1)
    return to_u8(ref), to_u8(tex), flow


def interior_epe(est, flow, h, w):
    """(mean, max) endpoint error over the interior, margin min(16, h // 4)"""
    m = min(16, h // 4)
    e = np.sqrt(((est.astype(np.float64) - flow) ** 2).sum(axis=0))[m:h - m, m:w - m]
    return float(e.mean()), float(e.max())
