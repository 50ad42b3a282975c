"""The temporal stabiliser (include/vstnet.h, "Stabiliser") stated in numpy fp64, in the kernel's order of operations: only + - * /,
comparisons and rint, each correctly rounded in both places, so the device must give the same bytes.  Also the bilinear warping
error the host tests judge a stabilised sequence by, and the two constructed clips of tests/test_stabilise_host.py."""
import numpy as np

DEFAULTS = dict(gain=0.7, sigma=8.0, limit=24.0)


def live_and_sample(flow, h, w, valid=None):
    """-> (live bool [h,w], x0, x1, y0, y1 int [h,w], ax, ay float64 [h,w]); the sample of a pixel that is not live is pixel (0, 0)
    with zero fractions: nothing is formed from its q"""
    f = np.asarray(flow, dtype=np.float32).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    with np.errstate(invalid="ignore"):
        qx, qy = xx - f[0], yy - f[1]
        inside = (qx >= 0.0) & (qx <= float(w - 1)) & (qy >= 0.0) & (qy <= float(h - 1))
    live = inside if valid is None else inside & (np.asarray(valid) != 0)
    cx = np.where(live, qx, 0.0)
    cy = np.where(live, qy, 0.0)
    cx = np.minimum(np.maximum(cx, 0.0), float(w - 1))
    cy = np.minimum(np.maximum(cy, 0.0), float(h - 1))
    x0 = np.clip(np.floor(cx).astype(np.int64), 0, w - 1)
    y0 = np.clip(np.floor(cy).astype(np.int64), 0, h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    return live, x0, x1, y0, y1, cx - x0.astype(np.float64), cy - y0.astype(np.float64)


def sample(frame_u8, x0, x1, y0, y1, ax, ay):
    """bilinear of a uint8 [h,w,3] frame on the 0..255 scale, float64 [h,w,3]: (1 - ay) ((1 - ax) a00 + ax a01) + ay ((1 - ax) a10
    + ax a11)"""
    a = frame_u8.astype(np.float64)
    ax, ay = ax[..., None], ay[..., None]
    top = (1.0 - ax) * a[y0, x0] + ax * a[y0, x1]
    bot = (1.0 - ax) * a[y1, x0] + ax * a[y1, x1]
    return (1.0 - ay) * top + ay * bot


def stabilise(cur_in, prev_in, cur_out, prev_written, flow, valid=None, gain=0.7, sigma=8.0, limit=24.0):
    """-> written uint8 [h,w,3]"""
    h, w = cur_out.shape[:2]
    live, x0, x1, y0, y1, ax, ay = live_and_sample(flow, h, w, valid)
    s = cur_out.astype(np.float64)
    i_w = sample(prev_in, x0, x1, y0, y1, ax, ay)
    o_w = sample(prev_written, x0, x1, y0, y1, ax, ay)
    d = cur_in.astype(np.float64) - i_w
    e = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / 3.0
    wgt = np.float64(gain) / (1.0 + e / (np.float64(sigma) * np.float64(sigma)))
    delta = np.minimum(np.maximum(wgt[..., None] * (o_w - s), -np.float64(limit)), np.float64(limit))
    blended = np.minimum(np.maximum(np.rint(s + delta), 0.0), 255.0).astype(np.uint8)
    return np.where(live[..., None], blended, cur_out)


def run_sequence(inputs, outputs, flows, valids=None, **params):
    """The recursion over a clip: frame 0, and a frame whose flow is None, is written as it is; frame t blends outputs[t] with
    what was written for frame t - 1.  flows[t] maps frame t - 1 onto frame t (flows[0] unused)."""
    written = [outputs[0].copy()]
    for t in range(1, len(outputs)):
        if flows[t] is None:
            written.append(outputs[t].copy())
        else:
            written.append(stabilise(inputs[t], inputs[t - 1], outputs[t], written[t - 1], flows[t],
                                     None if valids is None else valids[t], **params))
    return written


def warping_error(first, second, flow):
    """mean |bilinear(first; p - flow) - second| in levels over the pixels whose sample lies inside the frame"""
    h, w = second.shape[:2]
    live, x0, x1, y0, y1, ax, ay = live_and_sample(flow, h, w)
    diff = np.abs(sample(first, x0, x1, y0, y1, ax, ay) - second.astype(np.float64))
    return float(diff[live].mean())


def _to_u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def constructed_clip(kind, n=8, h=48, w=64, seed=0, noise=3.0, flicker=0.06):
    """-> (inputs, stylised, flows): n uint8 [h,w,3] input frames with independent Gaussian noise (sigma = `noise` levels), the
    "stylised" frames - a fixed colour map of the clean input, times the per-frame gain 1 + flicker (-1)^t, plus noise of their own
    - and the flows (flows[0] None).  The gain alternates on purpose: a gain drawn at random leaves some pairs with next to no
    change of gain, and on such a pair the ratio of the two warping errors shows the filter's memory of the frames before (the
    written frame still carries the gain of its predecessors), not how much flicker it damps; with the alternation every pair
    has the full step and the ratio is bounded by the filter alone: 1 - wgt on the first pair, less behind it.
    kind "static": one texture, zero flow.  kind "moving": a smooth sinusoidal texture under the constant flow (1.25, -0.5):
    frame t at p is the texture at p - t (1.25, -0.5)."""
    rng = np.random.default_rng(seed)
    fx, fy = (0.0, 0.0) if kind == "static" else (1.25, -0.5)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    phase = (0.0, 1.3, 2.1)

    def clean(t):
        x, y = xx - t * fx, yy - t * fy
        return np.stack([128.0 + 60.0 * np.sin(2 * np.pi * x / 23.0 + phase[c]) * np.cos(2 * np.pi * y / 17.0 - phase[c])
                         + 30.0 * np.sin(2 * np.pi * (x + y) / 41.0 + c) for c in range(3)], -1)

    inputs, stylised, flows = [], [], []
    for t in range(n):
        c = clean(t)
        inputs.append(_to_u8(c + rng.normal(0.0, noise, c.shape)))
        gain = 1.0 + flicker * (-1.0) ** t
        look = np.stack([0.9 * c[..., 0] + 10.0, 0.3 * c[..., 0] + 0.6 * c[..., 1], 255.0 - 0.8 * c[..., 2]], -1)
        stylised.append(_to_u8(gain * look + rng.normal(0.0, noise, c.shape)))
        flows.append(None if t == 0 else np.stack([np.full((h, w), fx), np.full((h, w), fy)]).astype(np.float32))
    return inputs, stylised, flows
