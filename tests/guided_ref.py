"""The yardstick of the guided upscale (vstnet.h, "Guided upscale"): numpy fp64 straight from the formulas, and the same with the
storage the kernels are allowed.  The box sums are plain sums of shifted copies (no summed-area table: nothing is subtracted);
the solve is numpy's.  Shared by tests/test_guided_host.py, tests/test_gpu_guided.py and tests/test_gpu_guided_pipeline.py."""
import numpy as np


def box_mean(x, r):
    """The mean over the (2 r + 1)^2 window clipped to the image, of every [h, w] plane of x (any leading axes)."""
    h, w = x.shape[-2:]
    pad = np.zeros(x.shape[:-2] + (h + 2 * r, w + 2 * r), np.float64)
    pad[..., r:r + h, r:r + w] = x
    acc = np.zeros(x.shape, np.float64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            acc += pad[..., dy:dy + h, dx:dx + w]
    ny = np.minimum(np.arange(h) + r, h - 1) - np.maximum(np.arange(h) - r, 0) + 1
    nx = np.minimum(np.arange(w) + r, w - 1) - np.maximum(np.arange(w) - r, 0) + 1
    return acc / (ny[:, None] * nx[None, :])


def guided_coef(G, P, r, eps):
    """G uint8 [h, w, 3], P float [3, h, w] -> the 12 smoothed coefficient planes, fp64: A[k][c] at 3 k + c, b[c] at 9 + c."""
    I = np.moveaxis(np.asarray(G, np.float64) / 255.0, 2, 0)                # [3, h, w]
    P = np.asarray(P, np.float64)
    mI, mP = box_mean(I, r), box_mean(P, r)
    sigma = box_mean(I[:, None] * I[None, :], r) - mI[:, None] * mI[None, :]           # [k, j, h, w]
    cov = box_mean(I[:, None] * P[None, :], r) - mI[:, None] * mP[None, :]             # [k, c, h, w]
    lhs = np.moveaxis(sigma, (0, 1), (2, 3)) + eps * np.eye(3)                         # [h, w, 3, 3]
    A = np.linalg.solve(lhs, np.moveaxis(cov, (0, 1), (2, 3)))                          # [h, w, k, c]
    b = np.moveaxis(mP, 0, 2) - np.einsum("hwkc,hwk->hwc", A, np.moveaxis(mI, 0, 2))
    planes = np.concatenate([np.moveaxis(A, (2, 3), (0, 1)).reshape(9, *A.shape[:2]), np.moveaxis(b, 2, 0)])
    return box_mean(planes, r)


def taps(n_full, n_small):
    """Half-pixel centres: (i0, i1, weight of i1) of every full-size index, in fp64."""
    v = np.clip((np.arange(n_full) + 0.5) * (n_small / n_full) - 0.5, 0.0, n_small - 1.0)
    i0 = np.floor(v).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_small - 1), v - i0


def quantise(q):
    """The writer's epilogue: * 255, clamp to [0, 255], truncate, NaN -> 0."""
    v = np.nan_to_num(np.asarray(q, np.float64) * 255.0, nan=0.0)
    return np.clip(v, 0.0, 255.0).astype(np.uint8)


def _apply(coef, S, dtype):
    H, W = S.shape[:2]
    h, w = coef.shape[1:]
    y0, y1, fy = taps(H, h)
    x0, x1, fx = taps(W, w)
    fy, fx = fy.astype(dtype)[:, None], fx.astype(dtype)[None, :]
    one = dtype(1)
    c = coef.astype(dtype)
    top = c[:, y0][:, :, x0] * (one - fx) + c[:, y0][:, :, x1] * fx
    bot = c[:, y1][:, :, x0] * (one - fx) + c[:, y1][:, :, x1] * fx
    s = top * (one - fy) + bot * fy                                                     # [12, H, W]
    I = np.moveaxis(S.astype(dtype) / dtype(255), 2, 0)
    q = s[9:12].copy()
    for k in range(3):
        q = q + s[3 * k:3 * k + 3] * I[k]
    return q


def guided_ref(G, P, S, r, eps, to_u8):
    """The guided upscale in fp64: guide G uint8 [h, w, 3], target P float [3, h, w], source S uint8 [H, W, 3] -> float64
    [3, H, W], or with to_u8 uint8 [H, W, 3] under the writer's epilogue."""
    q = _apply(guided_coef(G, P, r, eps), np.asarray(S), np.float64)
    return np.moveaxis(quantise(q), 0, 2) if to_u8 else q


def guided_emul(G, P, S, r, eps, to_u8):
    """guided_ref with the storage the kernels are allowed: the coefficient planes rounded to fp32 after the smoothing, the
    bilinear weights, the sampling and the affine apply in fp32 (coordinates stay fp64)."""
    q = _apply(guided_coef(G, P, r, eps).astype(np.float32), np.asarray(S), np.float32)
    return np.moveaxis(quantise(q), 0, 2) if to_u8 else q.astype(np.float64)


def brute_force(G, P, S, r, eps):
    """Four plain loops per pixel, for a tiny case: what guided_ref(..., to_u8=False) must give."""
    G, P, S = np.asarray(G), np.asarray(P, np.float64), np.asarray(S)
    h, w = G.shape[:2]
    H, W = S.shape[:2]
    I = G.astype(np.float64) / 255.0
    ab = np.zeros((h, w, 4, 3))
    for y in range(h):
        for x in range(w):
            pix = [(yy, xx) for yy in range(max(0, y - r), min(h - 1, y + r) + 1) for xx in range(max(0, x - r), min(w - 1, x + r) + 1)]
            Iw = np.array([I[p] for p in pix])
            Pw = np.array([P[:, p[0], p[1]] for p in pix])
            mI, mP = Iw.mean(0), Pw.mean(0)
            sigma = Iw.T @ Iw / len(pix) - np.outer(mI, mI)
            cov = Iw.T @ Pw / len(pix) - np.outer(mI, mP)
            A = np.linalg.inv(sigma + eps * np.eye(3)) @ cov
            ab[y, x, :3], ab[y, x, 3] = A, mP - A.T @ mI
    sm = np.zeros_like(ab)
    for y in range(h):
        for x in range(w):
            sm[y, x] = ab[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].mean((0, 1))
    out = np.zeros((3, H, W))
    for Y in range(H):
        for X in range(W):
            fy = min(max((Y + 0.5) * h / H - 0.5, 0.0), h - 1.0)
            fx = min(max((X + 0.5) * w / W - 0.5, 0.0), w - 1.0)
            y0, x0 = int(fy), int(fx)
            y1, x1 = min(y0 + 1, h - 1), min(x0 + 1, w - 1)
            fy, fx = fy - y0, fx - x0
            c = (sm[y0, x0] * (1 - fx) + sm[y0, x1] * fx) * (1 - fy) + (sm[y1, x0] * (1 - fx) + sm[y1, x1] * fx) * fy
            out[:, Y, X] = c[:3].T @ (S[Y, X] / 255.0) + c[3]
    return out


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
# (working size, full size, radius): tests/test_gpu_guided.py's table.  The kernels' workgroups are 256 columns of one row, at
# the working size (the four fit kernels) or at the full size (the apply).  For the apply, 408 full-size columns are more than
# one workgroup and no multiple of it, and a 77-column row of 231 bytes has a ragged last dword and rows that start off the dword
# grid.  For the fit, the table's working widths (at most 136) are all one workgroup, so the last case has a working frame of
# 300 columns: two workgroups per row, the second one partial, over several rows and - in the smoothing passes - 12 planes, which
# is the block index arithmetic a 1280-wide frame runs.  Every case has more than one row.
CASES = [((24, 36), (50, 77), 1), ((24, 36), (50, 77), 4), ((12, 16), (36, 48), 8), ((40, 136), (120, 408), 4),
         ((24, 36), (24, 36), 4), ((6, 300), (13, 610), 4)]
EPS = (1e-4, 1e-2)


def case_inputs(work_hw, full_hw, seed=0):
    """A seeded noise guide blended with a smooth ramp, P a smooth non-affine function of it plus noise, and a source frame of
    the full size in the same manner (the guide itself where the sizes are equal)."""
    rng = np.random.default_rng(1000 * work_hw[0] + work_hw[1] + 7 * full_hw[1] + seed)

    def frame(hw):
        y, x = np.mgrid[0:hw[0], 0:hw[1]]
        ramp = np.stack([x / hw[1], y / hw[0], (x + y) / (hw[0] + hw[1])], 2)
        return np.clip(255.0 * (0.6 * ramp + 0.4 * rng.random(hw + (3,))), 0, 255).astype(np.uint8)
    G = frame(work_hw)
    S = G if tuple(full_hw) == tuple(work_hw) else frame(full_hw)
    I = np.moveaxis(G.astype(np.float64) / 255.0, 2, 0)
    P = np.stack([np.sqrt(I[0] + 0.1) * 0.8, I[1] * I[2] + 0.2 * I[0], np.sin(2.0 * I[2]) * 0.5 + 0.3 * I[1] ** 2])
    P = (P + 0.02 * rng.standard_normal(P.shape)).astype(np.float32)
    return G, P, S


_cache = {}


def case(work_hw, full_hw, r, eps):
    """(G, P, S, guided_ref fp64 [3, H, W]) of one case: computed once, shared, read-only."""
    key = (tuple(work_hw), tuple(full_hw), r, eps)
    if key not in _cache:
        G, P, S = case_inputs(work_hw, full_hw)
        ref = guided_ref(G, P, S, r, eps, False)
        for a in (G, P, S, ref):
            a.setflags(write=False)
        _cache[key] = (G, P, S, ref)
    return _cache[key]


def emul_error():
    """max |guided_emul - guided_ref| over CASES x EPS, computed once (numpy only).  4 x this is the float budget of the GPU
    comparisons: the factor covers the order of the seven fp32 FMAs and of the bilinear weights, which the emulation fixes one
    way.  tests/test_guided_host.py prints it and checks it against the value recorded in profiles/guided_upscale.json."""
    if "emul" not in _cache:
        worst = 0.0
        for work_hw, full_hw, r in CASES:
            for eps in EPS:
                G, P, S, ref = case(work_hw, full_hw, r, eps)
                worst = max(worst, float(np.abs(guided_emul(G, P, S, r, eps, False) - ref).max()))
        _cache["emul"] = worst
    return _cache["emul"]


def float_budget():
    return 4.0 * emul_error()
