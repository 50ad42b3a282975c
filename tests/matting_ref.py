"""The yardstick of the affinity loss (csrc/matting.hip; vstnet.h, "Affinity loss") in numpy: the Matting-Laplacian quadratic form
as a window stencil, once in fp64 and once - the same formulas, the same function - in np.longdouble.

    window k (n = (2r+1)^2 pixels, centre at least r from every edge):  mu_k, S_k (population), inv_k = (S_k + (eps/n) 1)^-1, and
    per channel m_k, v_k = cov_k(I, x_c), a_k = inv_k v_k (solve="ldl": by L D L^T, the device's way; "adjugate": by cofactors)
    (L x_c)_i = sum_{k holds i} x_i - m_k - (I_i - mu_k)^T a_k        loss_c = sum_i x_i (L x_c)_i / (h w)        grad = 2 L x / (h w)
    closed_c  = sum_k n (var_k(x_c) - v_k^T a_k) / (h w)   (the same number, summed per window)

Moments are taken relative to the window's centre pixel, as on the device: a flat window has S_k = 0 exactly and a constant x
gives exactly 0.  `loss` is the sum over pixels, the form the device evaluates; `closed` is the per-window form of the issue,
which tests/test_matting_host.py holds against it and against the reference's own matrix (tests/golden/matting.npz)."""
import numpy as np

# (h, w, r).  The kernel's tiles are 16 x 16 (r = 1), 12 x 16 (r = 2) and 10 x 12 (r = 3) pixels: (37, 53, 1) is ragged against
# them, (70, 141, 2) has several tiles each way with ragged edges and halos across the seams, and (8, 4100, 1) is one row of 257
# tiles - more partial sums than the 256 threads of the second stage, so 4100 needs no raising.
CASES = [(3, 3, 1), (3, 40, 1), (40, 3, 1), (5, 5, 2), (7, 9, 3), (37, 53, 1), (70, 141, 2), (8, 4100, 1)]
CONTENT = {(37, 53, 1): "ramp", (70, 141, 2): "step"}         # every other case: white noise
EPS = 1e-7                                                     # the reference's default


def guide_of(h, w, kind, seed):
    """uint8 [h,w,3]: white noise; a ramp under +-3 counts of noise; or two exactly flat levels split down the middle column
    (windows away from the seam see a constant guide: the ridge alone)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        ramp = np.stack([200.0 * x / w + 20, 200.0 * y / h + 20, 100.0 * (x + y) / (h + w) + 60], 2)
        return np.clip(ramp + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    assert kind == "step"
    g = np.empty((h, w, 3), np.uint8)
    g[:, :w // 2] = (60, 90, 120)
    g[:, w // 2:] = (200, 150, 70)
    return g


AFFINE_M = np.array([[0.6, 0.2, -0.1], [0.05, 0.5, 0.2], [-0.1, 0.15, 0.7]])
AFFINE_C = np.array([0.1, 0.05, 0.12])


def x_of(G, kind, seed):
    """float32 [3,h,w]: uniform noise in [0,1); an exact affine function M I + c of the guide (rounded to fp32); a constant"""
    h, w = G.shape[:2]
    if kind == "noise":
        return np.random.default_rng(seed + 1).random((3, h, w)).astype(np.float32)
    if kind == "affine":
        return (np.einsum("ck,hwk->chw", AFFINE_M, G / 255.0) + AFFINE_C[:, None, None]).astype(np.float32)
    assert kind == "const"
    return np.ascontiguousarray(np.broadcast_to(np.array([0.25, 0.1, 0.7], np.float32)[:, None, None], (3, h, w)))


def as_u8(X):
    """a float frame as a written uint8 [h,w,3] frame (the writer's epilogue: * 255, clamp, truncate)"""
    return np.ascontiguousarray(np.moveaxis(np.clip(X * 255.0, 0, 255).astype(np.uint8), 0, 2))


def _windows(a, r):
    """[3,h,w] -> [3,h-2r,w-2r,n]: every window inside the image, at its centre's place less r"""
    d = 2 * r + 1
    v = np.lib.stride_tricks.sliding_window_view(a, (d, d), axis=(1, 2))
    return v.reshape(v.shape[0], v.shape[1], v.shape[2], d * d)


def matting(G, X, r=1, eps=EPS, dtype=np.float64, solve="ldl"):
    """G uint8 [h,w,3]; X float [3,h,w] or uint8 [h,w,3] (read as v / 255) -> dict(loss [3], closed [3], grad [3,h,w],
    scale [3]) in `dtype`; scale_c = sum_k n var_k(x_c) / (h w), the magnitude before the fit is taken off."""
    T = dtype
    h, w = G.shape[:2]
    n = (2 * r + 1) ** 2
    I = np.moveaxis(G.astype(T) / T(255), 2, 0)
    X = np.moveaxis(X.astype(T) / T(255), 2, 0) if X.dtype == np.uint8 else X.astype(T)
    assert I.shape == X.shape == (3, h, w) and h >= 2 * r + 1 and w >= 2 * r + 1
    mid = n // 2
    WI, WX = _windows(I, r), _windows(X, r)
    cI, cX = WI[..., mid], WX[..., mid]                                    # the centre pixels [3,ch,cw]
    dI, dX = WI - cI[..., None], WX - cX[..., None]
    mI, mX = dI.sum(-1) / T(n), dX.sum(-1) / T(n)                          # means, relative to the centre
    dI, dX = dI - mI[..., None], dX - mX[..., None]
    S = (dI[:, None] * dI[None, :]).sum(-1) / T(n)                         # [3,3,ch,cw]
    V = (dI[:, None] * dX[None, :]).sum(-1) / T(n)                         # [k,c,ch,cw] = cov(I_k, x_c)
    var = (dX * dX).sum(-1) / T(n)
    ridge = T(eps) / T(n)
    m00, m01, m02 = S[0, 0] + ridge, S[0, 1], S[0, 2]
    m11, m12, m22 = S[1, 1] + ridge, S[1, 2], S[2, 2] + ridge
    if solve == "ldl":
        # M = L D L^T (M is positive definite: the ridge), then two triangular solves - the device's way.  Its error grows with
        # the condition of M, (lambda_max + eps/n) / (eps/n), where the adjugate's grows with the square.
        i0 = T(1) / m00
        l10, l20 = m01 * i0, m02 * i0
        t = m12 - l20 * m01
        i1 = T(1) / (m11 - l10 * m01)
        l21 = t * i1
        i2 = T(1) / (m22 - l20 * m02 - l21 * t)
        z0 = V[0]
        z1 = V[1] - l10 * z0
        z2 = V[2] - l20 * z0 - l21 * z1
        a2 = z2 * i2
        a1 = z1 * i1 - l21 * a2
        a0 = z0 * i0 - l10 * a1 - l20 * a2
        A = np.stack([a0, a1, a2])                                         # [k,c,ch,cw]
    else:
        assert solve == "adjugate"
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        inv_det = T(1) / (m00 * c00 + m01 * c01 + m02 * c02)
        A = np.stack([(c00 * V[0] + c01 * V[1] + c02 * V[2]) * inv_det,
                      (c01 * V[0] + c11 * V[1] + c12 * V[2]) * inv_det,
                      (c02 * V[0] + c12 * V[1] + c22 * V[2]) * inv_det])   # [k,c,ch,cw]
    mu, q = cI + mI, cX + mX
    ch, cw = h - 2 * r, w - 2 * r
    Lx = np.zeros((3, h, w), T)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            Is, Xs = I[:, dy:dy + ch, dx:dx + cw], X[:, dy:dy + ch, dx:dx + cw]
            D = Is - mu
            Lx[:, dy:dy + ch, dx:dx + cw] += (Xs - q) - (D[0] * A[0] + D[1] * A[1] + D[2] * A[2])
    hw = T(h) * T(w)
    return {"loss": (X * Lx).sum((1, 2)) / hw,
            "closed": (T(n) * (var - (V * A).sum(0))).sum((1, 2)) / hw,
            "grad": T(2) * Lx / hw,
            "scale": (T(n) * var).sum((1, 2)) / hw}


# ------------------------------------------------------------------------------------------------ shared, computed once
_cache = {}


def case(h, w, r, x_kind="noise", u8=False):
    """(G, X, fp64 result) of one case; X is float32 [3,h,w] or, with u8, the uint8 [h,w,3] frame of it.  Read-only."""
    key = (h, w, r, x_kind, u8)
    if key not in _cache:
        G = guide_of(h, w, CONTENT.get((h, w, r), "noise"), 100 * h + w + r)
        X = x_of(G, x_kind, 100 * h + w + r)
        if u8:
            X = as_u8(X)
        ref = matting(G, X, r, EPS)
        for a in (G, X) + tuple(ref.values()):
            a.setflags(write=False)
        _cache[key] = (G, X, ref)
    return _cache[key]


X_FORMS = (("noise", False), ("noise", True), ("affine", False))    # (x, as a uint8 frame) the device tests run on every case


def float_error(twin="ldl"):
    """(loss, grad): the largest deviation of the fp64 evaluation from a longdouble evaluation of the same formulas over CASES x
    X_FORMS - the loss relative to the case's `scale`, the gradient absolute.  Computed once per twin.

    twin="adjugate" is the twin the issue names (the 3x3 inverse by the adjugate).  On the step case's windows across the seam -
    rank one, condition 1e7 - the adjugate loses the square of the condition, and in longdouble that is 2e-7 of the loss: more
    than the fp64 L D L^T solve loses.  twin="ldl" (the same solve, in longdouble) measures the fp64 arithmetic alone.  Both
    are printed by tests/test_matting_host.py; budgets() takes the smaller figure of each pair, so never more than the issue's."""
    key = ("err", twin)
    if key not in _cache:
        el = eg = 0.0
        for h, w, r in CASES:
            for kind, u8 in X_FORMS:
                G, X, ref = case(h, w, r, kind, u8)
                wide = matting(G, X, r, EPS, np.longdouble, twin)
                el = max(el, float(np.abs((ref["loss"] - wide["loss"]) / wide["scale"]).max()))
                eg = max(eg, float(np.abs(ref["grad"] - wide["grad"]).max()))
        _cache[key] = (el, eg)
    return _cache[key]


def budgets(max_abs_grad=None):
    """The device's budgets (loss relative to `scale`, gradient absolute): 16 x float_error(), for another summation order and
    FMA contraction; for the float32 gradient plus half an ulp of float32 at max |grad|."""
    (la, ga), (ll, gl) = float_error("adjugate"), float_error("ldl")
    bl, bg = 16.0 * min(la, ll), 16.0 * min(ga, gl)
    if max_abs_grad is not None:
        bg += 0.5 * float(np.spacing(np.float32(max_abs_grad)))
    return bl, bg
