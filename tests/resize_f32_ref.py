"""The antialiased float resize of csrc/resize.hip (vst_resize_f32, vst_resize_f32_to_u8) in float64 with an element-wise
bound on the fp32 kernels' error, and an fp32 emulation of the kernels to plant faults in (helpers of test_resize_host.py /
test_gpu_resize_f32.py).

Reference: two passes with ``resize_ref.aa_weights_f64``, horizontal first, on the float32 input taken exactly.  With W1, W2 the
passes as matrices, t = W1 x, n the taps of an output and u = 2^-24:

    E1 = (n1 + 2) u (|W1| |x|)                      E = (n2 + 2) u (|W2| |t|) + |W2| E1

n fma roundings (each at most u times a partial sum, which |W| |x| bounds), one rounding of the stored coefficient, one for the
second-order terms.  Where the width does not change there is no horizontal pass (E1 = 0); the vertical pass always runs, with
its identity table where the height does not change.
"""
import numpy as np

from tests import resize_ref

U = 2.0 ** -24
H_ROWS = 8

# (Hs, Ws) -> (Hd, Wd), B = 2 throughout: what each reaches is in test_gpu_resize_f32.py
CASES = [((5, 7), (11, 13)), ((9, 130), (7, 127)), ((13, 40), (8, 260)), ((64, 48), (4, 3)), ((1, 1), (3, 5)), ((17, 33), (17, 9)),
         ((17, 33), (6, 33)), ((11, 350), (23, 343)), ((33, 19), (5, 19))]
B = 2


def table(in_size, out_size, fault=None):
    """(ksize, bounds [out,2], w float64 [out,ksize]) as vst_resize_coeffs_f32 builds it before rounding to float32, or with a
    planted fault: `reciprocal` (t * (1 / filterscale) for t / filterscale), `border` (a window cut by the frame's edge keeps the
    normalisation of the whole window)"""
    if fault not in ("reciprocal", "border"):
        return resize_ref.aa_weights_f64(in_size, out_size)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    ksize = resize_ref.ksize_of(in_size, out_size)
    bounds, kk = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ksize), np.float64)
    arg = (lambda t: t * ss) if fault == "reciprocal" else (lambda t: t / fs)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo, hi = int(center - support + 0.5), int(center + support + 0.5)
        xmin, xmax = max(lo, 0), min(hi, in_size)
        w = [resize_ref.cubic(arg(x - center + 0.5)) for x in range(xmin, xmax)]
        ww = sum(w) if fault == "reciprocal" else sum(resize_ref.cubic(arg(x - center + 0.5)) for x in range(lo, hi))
        bounds[xx] = (xmin, xmax - xmin)
        kk[xx, :xmax - xmin] = [v / ww for v in w]
    return ksize, bounds, kk


def _matrix(in_size, out_size):
    _, bounds, w = resize_ref.aa_weights_f64(in_size, out_size)
    m = np.zeros((out_size, in_size), np.float64)
    for i, (first, n) in enumerate(bounds):
        m[i, first:first + n] = w[i, :n]
    return m, bounds[:, 1].astype(np.float64)


def frames(src_hw, seed):
    """float32 [B,3,Hs,Ws] in [-0.1, 1.1]: both clamps of the byte form are reached"""
    return (np.random.default_rng(seed).random((B, 3) + tuple(src_hw)) * 1.2 - 0.1).astype(np.float32)


def reference(x, dst_hw):
    """x float32 [B,3,Hs,Ws] -> (ref, E) float64 [B,3,Hd,Wd]"""
    assert x.dtype == np.float32
    x = x.astype(np.float64)
    Hd, Wd = dst_hw
    Hs, Ws = x.shape[2:]
    if Ws != Wd:
        m1, n1 = _matrix(Ws, Wd)
        t = x @ m1.T
        e1 = (n1 + 2.0) * U * (np.abs(x) @ np.abs(m1).T)
    else:
        t, e1 = x, np.zeros_like(x)
    m2, n2 = _matrix(Hs, Hd)
    ref = np.einsum("yh,bchx->bcyx", m2, t)
    e = (n2 + 2.0)[None, None, :, None] * U * np.einsum("yh,bchx->bcyx", np.abs(m2), np.abs(t)) + \
        np.einsum("yh,bchx->bcyx", np.abs(m2), e1)
    return ref, e


def to_bytes(ref, e):
    """the byte form's criterion for [B,3,Hd,Wd] -> HWC: (lowest, reference, highest) byte of (uint8)clamp(255 v) for v within
    e of ref, the * 255 rounded once more; and where 255 ref is within that of an integer"""
    t = np.transpose(ref, (0, 2, 3, 1)) * 255.0
    et = np.transpose(e, (0, 2, 3, 1)) * 255.0 + np.abs(t) * U
    q = lambda v: np.floor(np.clip(v, 0.0, 255.0)).astype(np.int64)          # noqa: E731
    return q(t - et), q(t), q(t + et), np.abs(t - np.rint(t)) <= et


def check_float(got, ref, e):
    """-> (ok, worst error / E)"""
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    return err <= e, float((err / e).max())


def check_bytes(got, ref, e):
    """-> (ok, bytes that differ from the reference's, largest difference): within one count of trunc(clamp(255 ref)) and a
    byte the epilogue can give for a value within E, which lets a byte differ only where 255 ref is within 255 E + 255 |ref| u
    of an integer"""
    lo, mid, hi, _ = to_bytes(ref, e)
    assert got.dtype == np.uint8 and got.shape == mid.shape, (got.dtype, got.shape, mid.shape)
    d = got.astype(np.int64)
    return (lo <= d) & (d <= hi) & (np.abs(d - mid) <= 1), int((d != mid).sum()), int(np.abs(d - mid).max())


# ------------------------------------------------------------------------------------------------ the kernels in numpy float32
def _fma32(acc, v, c):
    """fmaf(v, c, acc): the product of two float32 is exact in float64, the sum is rounded there and once more to float32"""
    return (acc.astype(np.float64) + v.astype(np.float64) * c.astype(np.float64)).astype(np.float32)


def _pass32(src, tab, fault):
    """one pass along the last axis of src [rows, in] with a table -> [rows, out]: the taps in order, one fma each"""
    ksize, bounds, w = tab
    w32 = w.astype(np.float32)
    first, n = bounds[:, 0].astype(np.int64), bounds[:, 1]
    if fault == "first":
        first = np.minimum(first + 1, src.shape[1] - 1)
    acc = np.zeros((src.shape[0], len(first)), np.float32)
    for j in range(ksize):
        idx = np.minimum(first + j, src.shape[1] - 1)
        acc = np.where((j < n)[None, :], _fma32(acc, src[:, idx], w32[None, :, j]), acc)
    return acc


def emulate(x, dst_hw, fault=None):
    """vst_resize_f32 in numpy: float32 [B,3,Hd,Wd].  Faults: `rows` (the horizontal pass addresses a plane's rows as if
    every plane held a whole number of H_ROWS row groups, so the rows behind a plane's last full group come from the next
    plane), `first` (every window starts one tap late), `border`, `reciprocal` (see table)."""
    assert x.dtype == np.float32
    Bn, C, Hs, Ws = x.shape
    Hd, Wd = dst_hw
    tf = fault if fault in ("border", "reciprocal") else None
    t = x
    if Ws != Wd:
        rows = x.reshape(Bn * C * Hs, Ws)
        if fault == "rows":
            pitch = (Hs + H_ROWS - 1) // H_ROWS * H_ROWS
            flat = (np.arange(Bn * C)[:, None] * pitch + np.arange(Hs)[None, :]).reshape(-1)
            rows = rows[np.minimum(flat, len(rows) - 1)]
        t = _pass32(rows, table(Ws, Wd, tf), fault).reshape(Bn, C, Hs, Wd)
    cols = np.ascontiguousarray(np.moveaxis(t, 2, 3)).reshape(Bn * C * Wd, Hs)
    out = _pass32(cols, table(Hs, Hd, tf), fault).reshape(Bn, C, Wd, Hd)
    return np.ascontiguousarray(np.moveaxis(out, 3, 2))


def quantise(out32, fault=None):
    """resize_v_f32_u8_kernel's epilogue: * 255 in float32, clamp, truncate, HWC"""
    t = np.clip(np.transpose(out32, (0, 2, 3, 1)) * np.float32(255.0), np.float32(0.0), np.float32(255.0))
    return np.ascontiguousarray((np.rint(t) if fault == "round" else np.trunc(t)).astype(np.uint8))


_cache = {}


def case(i):
    """(x, ref, E) of CASES[i], built once per process"""
    if i not in _cache:
        src, dst = CASES[i]
        x = frames(src, seed=100 + i)
        ref, e = reference(x, dst)
        for a in (x, ref, e):
            a.setflags(write=False)
        _cache[i] = (x, ref, e)
    return _cache[i]
