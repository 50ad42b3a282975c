"""Host restatements for the style-map tests ("Style maps"; include/vstnet.h, "Style maps").

  * weight_rows: K weight planes in ROW order, so that most 32-row tiles of the packed kernels mix the kinds of row the issue
    names (exact one-hot rows for each k, multiples of 1/255, arbitrary floats normalised, a run of 256 consecutive one-hot rows
    that starts at row 8 and one that straddles the two halves);
  * mix64 / mix32: sum_k w_k (T_k x + t0_k) in fp64 with its condition-like denominator, and the one-thread fp32 restatement of
    the device's arithmetic (a_k as cwct_ops_ref.apply32 restates the plain apply, then m = w_0 a_0, m = m + w_k a_k), with two
    mutants: the weights of rows swapped between k = 0 and k = 1, and t0_k added unweighted;
  * loader_weights: the weight arithmetic of --style_map / --style_maps from 8-bit planes.
No GPU is needed to import or run anything here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cwct_ops_ref as O                                               # noqa: E402

MUTANTS = ("weights_swapped", "t0_unweighted")
MIX_CASES = [(32, 2, 260), (32, 3, 66), (32, 8, 260), (128, 2, 130)]     # (N, K, rows): partial tiles, more than one tile


def weight_rows(rows, K, seed):
    """float32 [K, rows] in row order, every row >= 0 and summing to 1 within a few ulp"""
    rng = np.random.default_rng([seed, K, rows])
    kind = rng.integers(0, 3, rows)
    hot = rng.integers(0, K, rows)
    w = rng.random((K, rows), dtype=np.float32) + np.float32(1e-3)
    w = (w / w.sum(axis=0, dtype=np.float32)).astype(np.float32)
    # multiples of 1/255 that sum to 255: K - 1 cuts of 0..255
    cuts = np.sort(rng.integers(0, 256, (K - 1, rows)), axis=0)
    v = np.diff(np.concatenate([np.zeros((1, rows), np.int64), cuts, np.full((1, rows), 255, np.int64)]), axis=0)
    w = np.where(kind[None] == 1, v.astype(np.float32) / np.float32(255), w)
    onehot = (np.arange(K)[:, None] == hot[None]).astype(np.float32)
    w = np.where(kind[None] == 0, onehot, w).astype(np.float32)
    blk = 256 if rows >= 784 else rows // 4
    w[:, 8:8 + blk] = 0.0
    w[seed % K, 8:8 + blk] = 1.0
    a = rows // 2 - blk // 2
    w[:, a:a + blk] = 0.0
    w[(seed + 1) % K, a:a + blk] = 1.0
    return np.ascontiguousarray(w)


def mix64(x, affs, w, N):
    """x [N, L], affs [K, N*N+N], w [K, L] -> (sum_k w_k (T_k x + t0_k), sum_k w_k (|T_k| |x| + |t0_k|)) in fp64"""
    want = np.zeros(x.shape, np.float64)
    den = np.zeros(x.shape, np.float64)
    for k in range(len(affs)):
        a, d = O.apply64(x, affs[k], N)
        wk = np.asarray(w[k], np.float64)[None]
        want += wk * a
        den += wk * d
    return want, den


def mix32(x, affs, w, N, mut=()):
    """the device's arithmetic, one rounding per operation: a_k = the plain apply's restatement, m = w_0 a_0, m = m + w_k a_k"""
    w = np.asarray(w, np.float32)
    if "weights_swapped" in mut:
        w = w.copy()
        w[[0, 1]] = w[[1, 0]]
    m = None
    for k in range(len(affs)):
        if "t0_unweighted" in mut:
            a = O.apply32(x, affs[k], N, mut=("t0_not_added",))
        else:
            a = O.apply32(x, affs[k], N)
        p = (w[k][None] * a).astype(np.float32)
        m = p if m is None else (m + p).astype(np.float32)
    if "t0_unweighted" in mut:
        for k in range(len(affs)):
            m = (m + affs[k][N * N:][:, None]).astype(np.float32)
    return m


def mix_input(N, K, rows, seed=0):
    """x [N, rows], K affines, weights [K, rows]: cwct_ops_ref's inputs (|T| over four decades, a zero row, a zero pixel)"""
    x = O.apply_input(N, rows, seed=seed)[0]
    affs = np.ascontiguousarray(O.affines_input(N, K, seed=seed)[:K])
    return x, affs, weight_rows(rows, K, seed + 3)


def loader_weights(planes):
    """planes: list of uint8 [h, w] arrays at the code's resolution -> float32 [K, h, w].  One plane: t = v / 255, w = (1 - t, t).
    K planes: w_k = v_k / sum_j v_j with the sum taken in integers.  A pixel whose planes are all 0 raises ValueError."""
    planes = [np.asarray(p, np.uint8) for p in planes]
    if len(planes) == 1:
        t = planes[0].astype(np.float32) / np.float32(255)
        return np.stack([np.float32(1) - t, t])
    tot = np.zeros(planes[0].shape, np.int64)
    for p in planes:
        tot += p
    if (tot == 0).any():
        y, x = np.argwhere(tot == 0)[0]
        raise ValueError(f"every plane is 0 at pixel (x={x}, y={y})")
    return np.stack([p.astype(np.float32) / tot.astype(np.float32) for p in planes])
