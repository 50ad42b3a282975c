"""References, host restatements, mutants, launch conditions and case tables of the per-kernel tests of csrc/cwct_any.hip (the
fp32 `_n` family, N = 1..256) and csrc/cwct64.hip (the `use_double` route: `_f64` at the tuned widths, `_n_f64` at any width).
Test infrastructure only (tests/test_cwct_any_host.py, tests/test_gpu_cwct_ops_any.py); imports no GPU code.

fp32 `_n` family.  cwct_any.hip has the tuned kernels' records, group rule and arithmetic, so the references (O.stats64,
O.factor64, O.apply64), the restatements (O.stats32 / O.combine, O.factor32, O.apply32: all take N as an argument), the normalised
metrics and the bound of tests/cwct_ops_ref.py (`O`) are used as they are: device error <= O.FACTOR[op] x max(e32, O.FLOOR[op]).
stats32_n and apply32_n are those restatements with the switches of this family's mutants; without a switch they return O's bits.

fp64 families.  Reference: the same mathematics in np.longdouble (64-bit mantissa; the host test refuses a machine where it
is not): two-pass statistics, a column Cholesky with the reference's cumulative jitter (every step eps, 2 eps, ... rounded to
fp32 as the float32 identity times eps is), triangular inverse, T = mixL Lc^-1, t0 = mix_mean - T mean_c, y = T x + t0.
Restatement (e64): the kernels' documented arithmetic in numpy float64 - per-2048-pixel chunk sums added in index order, centred
products summed over a chunk's pixels in index order and the chunks in index order, the right-looking fp64 Cholesky (its update
one rounding, through longdouble), the row-by-row triangular inverse, M Li, fp64 accumulation of the apply.  Bounds:
  statistics, factor : error <= FACTOR64 x max(e64, 2^-53) under O's normalised metrics;
  apply (one rounding to fp32): |y - y_ref| <= ulp32(y_ref) / 2 + FACTOR64 x max(e64, 2^-53) x (sum |T||x| + |t0|).
FACTOR64 = 4 for the reason O gives for FACTOR: two evaluations of one sum in different orders each err by about e, and the
device gets twice their distance.  The floor is fp64's unit roundoff.  apply64_ratio folds the apply bound into one figure:
max over ALL elements of (|y - y_ref| - ulp32 / 2) / (max(e64, 2^-53) den), to be <= FACTOR64.

Mutants are switches on the restatements; each must exceed 1.25 x the factor at one case of the tables (the host test asserts it
and prints the figures).  "pad_channel_not_zeroed" is a mutant of the apply only: in the statistics kernels a channel >= N of a
padded block reaches only co-moment entries that are never written, so zeroing it or not cannot be observed there.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cwct_ops_ref as O                                               # noqa: E402

LD = np.longdouble
U64 = 2.0 ** -53
FACTOR64 = 4.0
CHUNK = 2048                      # CWCT64_CHUNK: pixels per workgroup of the fp64 statistics passes


def ratio64(err, e64):
    return err / max(e64, U64)


# ================================================================================================== launch conditions
def stats_n_form(N):
    """vst_cwct_stats_n: which kernel, and for the tile kernels how many channel blocks (TN = 16 RB channels each)"""
    if N <= 4:
        return "reg4"
    if N <= 8:
        return "reg8"
    if N <= 16:
        return "reg16"
    if N <= 32:
        return "tile2"
    return f"tile4x{(N + 63) // 64}"


def stats_n_block(N):
    """channels per block of the tile kernels (0: the register kernels have no blocks)"""
    return 0 if N <= 16 else (32 if N <= 32 else 64)


def apply_n_form(N):
    """cwctn_apply_launch: (PG = 64-pixel groups per workgroup, dynamic LDS bytes, has a partial column block)"""
    NP = (N + 15) & ~15
    PG = 4 if NP <= 32 else (2 if NP <= 64 else 1)
    return PG, NP * 64 * PG * 4, N % 16 != 0


def cov64n_blocks(N):
    """gridDim.y of stats64n_cov_kernel: 1024 pairs per workgroup"""
    return (N * N + 1023) // 1024


def chunks64(L):
    return (L + CHUNK - 1) // CHUNK


# ============================================================================================================= inputs
def skip_ch(N):
    return (O.CONST_CH,) if N >= 3 else ()


def stats_input_n(N, L, kind="scales", seed=0):
    """O.stats_input; below 3 channels its first channels without the collinear and the constant one"""
    if N >= 3:
        return O.stats_input(N, L, kind, seed)
    return np.ascontiguousarray(O.stats_input(4, L, kind, seed)[[0, 3][:N]])


def long_input_n(N, L):
    """O.long_input at N channels"""
    import torch
    scales = torch.logspace(-2, math.log10(3.0), N, dtype=torch.float32)[:, None]
    x = np.empty((N, L), dtype=np.float32)
    ch = 1 << 18
    for k in range(-(-L // ch)):
        a, b = k * ch, min((k + 1) * ch, L)
        g = torch.Generator().manual_seed(77 + k)
        x[:, a:b] = (50.0 + scales * torch.randn(N, b - a, generator=g, dtype=torch.float32)).numpy()
    if N >= 3:
        x[O.CONST_CH] = O.CONST_VAL
    return x


def apply_input_n(N, L, seed=0, f64=False):
    """O.apply_input (a zero pixel, a zero row where there is a second row, |T| over four decades); f64: the affine keeps its
    fp64 bits (x stays float32)"""
    if N >= 2 and not f64:
        return O.apply_input(N, L, seed)
    g = np.random.RandomState(31 * N + L % 9973 + seed)
    x = (g.randn(N, L) * np.logspace(-1, 1, N)[:, None]).astype(np.float32)
    x[:, O.ZERO_PIXEL] = 0.0
    T = g.randn(N, N) * 10.0 ** g.uniform(-3, 1, (N, N))
    if N >= 2:
        T[O.ZERO_ROW] = 0.0
    aff = np.concatenate([T.reshape(-1), g.randn(N) * 3.0])
    return x, (aff if f64 else aff.astype(np.float32))


# ======================================================================================================== fp32, `_n`
def stats32_n(x, mask=None, label=0, mut=()):
    """O.stats32 at the groups of O.stats_groups, with this family's switches"""
    N, L = x.shape
    g, per, _ = O.stats_groups(L)
    TN = stats_n_block(N)
    blk = np.arange(N) // TN if TN else np.zeros(N, dtype=int)
    recs = []
    with O.one_thread():
        for w in range(g):
            a, b = w * per, min((w + 1) * per, L)
            sel = slice(None)
            if mask is not None:
                sel = mask[a:b] == label
                if "mask_ignored_last_tile" in mut:
                    sel = sel.copy()
                    sel[(b - a - 1) // 64 * 64:] = True
            n, sh, asum, q = O._group_record(x[:, a:b], sel, ())
            if "pair_one_sided" in mut:                    # the mirrored write of every pair bi < bj is missing
                q = np.where(blk[:, None] > blk[None, :], np.float32(0.0), q)
            if "diag_sums_missing" in mut and TN:          # the last diagonal pair does not write its channels' sums
                asum = asum.copy()
                asum[(N - 1) // TN * TN:] = 0.0
            if "count_missing" in mut:
                n = 0.0
            recs.append((n, sh, asum, q))
    return O.combine(recs, N)


def _with_pad(x, aff, N, mut):
    """the apply's switches that act on its inputs: the columns of the last partial 16-column block"""
    T = aff[:N * N].reshape(N, N).copy()
    full = N // 16 * 16
    extra = None
    if "partial_block_dropped" in mut:
        T[:, full:] = 0.0
    if "pad_channel_not_zeroed" in mut and N % 16:
        # the partial block run as a full one over rows of the staging buffer that were not zeroed: columns N .. NP - 1 take
        # the affine's next words (row i + 1 of T, or t0) and whatever the buffer held, here the first channels of x
        NP = (N + 15) // 16 * 16
        flat = np.concatenate([aff, np.zeros(NP, dtype=aff.dtype)])
        idx = np.arange(N)[:, None] * N + np.arange(N, NP)[None, :]
        extra = flat[idx] @ x[(np.arange(N, NP) - N) % N].astype(aff.dtype)
    return np.concatenate([T.reshape(-1), aff[N * N:]]), extra


def apply32_n(x, aff, N, mut=()):
    a2, extra = _with_pad(x, aff, N, mut)
    y = O.apply32(x, a2, N, mut=tuple(m for m in mut if m == "t0_not_added"))
    return y if extra is None else (y + extra.astype(np.float32)).astype(np.float32)


# ============================================================================================================== fp64
def pack_ld(n, mean, cov):
    return np.concatenate([np.array([n], dtype=LD), np.asarray(mean, dtype=LD), np.asarray(cov, dtype=LD).reshape(-1)])


def stats_ld(x, sel=None):
    """two-pass longdouble record of the columns of x that `sel` picks"""
    cols = (x if sel is None else x[:, sel]).astype(LD)
    n = cols.shape[1]
    mean = cols.sum(1) / LD(n)
    d = cols - mean[:, None]
    return pack_ld(n, mean, d @ d.T / LD(n - 1.0))


def stats_e64(x, sel=None, mut=()):
    """restatement of stats64(n)_sum / mean / cov / cov_combine in float64"""
    N, L = x.shape
    on = np.ones(L, dtype=bool) if sel is None else sel
    cols = [x[:, a:a + CHUNK][:, on[a:a + CHUNK]].astype(np.float64) for a in range(0, L, CHUNK)]
    s, n = np.zeros(N), 0.0
    for c in cols:
        s = s + c.sum(1)
        n += c.shape[1]
    mean = s / n
    if "mean_fp32" in mut:
        mean = mean.astype(np.float32).astype(np.float64)
    m2 = np.zeros((N, N))
    for c in cols:
        d = c - mean[:, None]
        if "centred_fp32" in mut:
            d = d.astype(np.float32).astype(np.float64)
        acc = np.zeros((N, N))
        for p in range(d.shape[1]):
            acc += d[:, p, None] * d[None, :, p]
        m2 = m2 + acc
    return O.pack(n, mean, m2 / (n - 1.0))


def stats64_ratio(got, e64rec, want, N, skip=()):
    """the larger of the covariance and the mean ratio, each against its own e64 (O.stats_ratio with fp64's floor)"""
    (gc, gm), (ec, em) = O.stats_err(got, want, N, skip), O.stats_err(e64rec, want, N, skip)
    return max(ratio64(gc, ec), ratio64(gm, em)), (gc, gm, ec, em)


def jitter_steps(tries, eps):
    """eps, 2 eps, ... each rounded to fp32 (chol64; cWCT.py's float32 identity times eps)"""
    e = float(np.float32(eps))
    return [float(np.float32(float(t) * e)) for t in range(1, tries + 1)]


def chol_ld(a):
    """column Cholesky in longdouble; None where a pivot is not positive"""
    a = a.astype(LD).copy()
    n = a.shape[0]
    for j in range(n):
        d = a[j, j] - a[j, :j] @ a[j, :j]
        if not d > 0:
            return None
        a[j, j] = np.sqrt(d)
        a[j + 1:, j] = (a[j + 1:, j] - a[j + 1:, :j] @ a[j, :j]) / a[j, j]
    return np.tril(a)


def inv_lower(L):
    """inverse of a lower triangular matrix, row by row, in L's own type"""
    n = L.shape[0]
    Li = np.zeros_like(L)
    for i in range(n):
        Li[i, i] = 1.0 / L[i, i]
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
    return Li


def factor_ld(content, styles, alphas, alpha_c, N, tries, eps=O.EPS):
    """the factor in longdouble with the jitter the given retry counts add: (T, t0, denominators), as O.factor64"""
    def chol(rec, t):
        cnt, _, cov = O.unpack(rec, N)
        if cnt < 0:
            return cov.astype(LD)
        a = cov.astype(LD)
        for st in jitter_steps(t, eps):
            a = a + np.eye(N, dtype=LD) * LD(st)
        return chol_ld(a)
    mixL, mixmu = np.zeros((N, N), dtype=LD), np.zeros(N, dtype=LD)
    for s, (rec, al) in enumerate(zip(styles, alphas)):
        al = LD(float(np.float32(al)))
        mixL = mixL + chol(rec, tries[2 + s]) * al
        mixmu = mixmu + O.unpack(rec, N)[1].astype(LD) * al
    Lc = chol(content, tries[0])
    cmean = O.unpack(content, N)[1].astype(LD)
    if alpha_c != 0.0:
        ac = LD(float(np.float32(alpha_c)))
        mixL = mixL * (1 - ac) + Lc * ac
        mixmu = mixmu * (1 - ac) + cmean * ac
    Li = inv_lower(Lc)
    T = mixL @ Li
    dT = np.abs(mixL) @ np.abs(Li)
    return T, mixmu - T @ cmean, dT, np.abs(mixmu) + dT @ np.abs(cmean)


def chol_e64(a):
    """right-looking float64 Cholesky with LAPACK's failure rule (chol64): (L, failed); the rank-1 update is rounded once"""
    a = a.copy()
    n = a.shape[0]
    for j in range(n):
        d = a[j, j]
        if not d > 0:
            return None, True
        p = np.sqrt(d)
        col = a[j + 1:, j] / p
        a[j, j] = p
        a[j + 1:, j] = col
        c = col.astype(LD)
        a[j + 1:, j + 1:] = (a[j + 1:, j + 1:].astype(LD) - np.outer(c, c)).astype(np.float64)
    return np.tril(a), False


def factor_chol_e64(rec, N, eps, min_tries=0, mut=()):
    cnt, _, cov = O.unpack(rec, N)
    if cnt < 0:
        return cov.copy(), 0
    tries = max(0, min_tries)
    while True:
        a = cov.copy()
        d = np.diag(a).copy()
        steps = jitter_steps(tries, eps)
        for st in (steps[-1:] if "jitter_not_cumulative" in mut else steps):
            d = d + st
        a[np.diag_indices_from(a)] = d
        L, failed = chol_e64(a)
        if not failed:
            return L, tries
        tries += 1


def factor_e64(content, styles, alphas, alpha_c, N, eps=O.EPS, min_tries=None, mut=()):
    """restatement of cwct_factor64_kernel in float64: (affine float64 [N*N + N], info [2 + n_styles])"""
    k = len(styles)
    mt = list(min_tries) if min_tries is not None else [0] * (2 + k)
    info = [0] * (2 + k)
    M, mixmu = np.zeros((N, N)), np.zeros(N)
    for s, (rec, al) in enumerate(zip(styles, alphas)):
        Ls, info[2 + s] = factor_chol_e64(rec, N, eps, mt[2 + s], mut)
        al = float(np.float32(al))
        M = M + Ls * al
        mixmu = mixmu + O.unpack(rec, N)[1] * al
    Lc, info[0] = factor_chol_e64(content, N, eps, mt[0], mut)
    cmean = O.unpack(content, N)[1]
    if alpha_c != 0.0:
        ac = float(np.float32(alpha_c))
        M = M * (1.0 - ac) + Lc * ac
        mixmu = mixmu * (1.0 - ac) + cmean * ac
    T = np.tril(M @ inv_lower(Lc))
    return np.concatenate([T.reshape(-1), mixmu - T @ cmean]), info


def apply_ld(x, aff, N):
    aff = np.asarray(aff).astype(LD)
    T, t0 = aff[:N * N].reshape(N, N), aff[N * N:]
    x = np.asarray(x).astype(LD)
    return T @ x + t0[:, None], np.abs(T) @ np.abs(x) + np.abs(t0)[:, None]


def apply_e64(x, aff, N, mut=()):
    """restatement of cwct_apply64_kernel / cwctn_apply_kernel<double>: the float64 value before its one rounding to fp32"""
    aff = np.asarray(aff, dtype=np.float64)
    a2, extra = _with_pad(x, aff, N, mut)
    T, t0 = a2[:N * N].reshape(N, N), a2[N * N:]
    if "T_fp32" in mut:
        T = T.astype(np.float32).astype(np.float64)
    y = T @ np.asarray(x, dtype=np.float64)
    if "t0_not_added" not in mut:
        y = y + t0[:, None]
    return y if extra is None else y + extra


def half_ulp32(y):
    """half the spacing of float32 in the binade of |y| (y longdouble): what one rounding to nearest may cost"""
    _, e = np.frexp(np.abs(np.asarray(y, dtype=np.float64)))
    return np.ldexp(0.5, np.maximum(e - 24, -149))


def apply64_ratio(got, e64, want, den):
    """max over every element of (|got - want| - ulp32 / 2) / (max(e64, 2^-53) den); an element with den = 0 must be exact"""
    err = np.abs(np.asarray(got).astype(LD) - want)
    err = np.where(np.isfinite(err), err, np.inf)
    rest = np.maximum(err - half_ulp32(want), 0.0)
    scale = max(e64, U64) * den
    r = np.where(scale > 0, rest / np.where(scale > 0, scale, 1.0), np.where(rest > 0, np.inf, 0.0))
    return float(r.max())


def apply64_e64(y64, want, den):
    return O.apply_err(y64, want, den)


# ======================================================================================================== case tables
STATS_N_WIDTHS = {"reg4": (1, 3, 4), "reg8": (5, 8), "reg16": (9, 12, 16), "tile2": (17, 24, 32), "tile4x1": (33, 48, 64),
                  "tile4x2": (65, 100, 128), "tile4x3": (129, 160, 192), "tile4x4": (193, 255, 256)}
STATS_N = tuple(n for ws in STATS_N_WIDTHS.values() for n in ws)
STATS_OFFS = (0, 1)
STATS_N_CASES = [(N, L, "scales") for N in STATS_N for L in O.STATS_L] + [(N, 1729, "outlier") for N in STATS_N]
MASK_N_CASES = [(N, L) for N in STATS_N for L in O.MASK_L]
MASK_OFFS = (0, 1)
LONG_N_CASES = [(5, (1 << 21) + 68), (17, (1 << 18) + 68), (17, (1 << 19) + 68), (17, (1 << 21) + 68)]

FACTOR_N = (1, 3, 12, 24, 48, 100, 160, 256)
FACTOR_N_CASES = [(N, k, ac, cond) for N in FACTOR_N for k in (1, 2, 8) for ac in (0.0, 0.3) for cond in (1e1, 1e4)
                  if not (N == 256 and k == 8)]
JITTER_N = (12, 24, 100)
GIVE_UP_N = (1, 4)

APPLY_N = (1, 15, 16, 17, 31, 32, 33, 48, 64, 65, 100, 240, 241, 256)
APPLY_L = (1, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260)
APPLY_N_CASES = [(N, L, masked) for N in APPLY_N for L in APPLY_L for masked in (False, True)]
TUNED = (16, 32, 64, 128)

F64_N = {"f64": (16, 32, 64, 128), "n_f64": (1, 3, 24, 32, 33, 100, 256)}
F64_FAMILIES = [(fam, N) for fam in ("f64", "n_f64") for N in F64_N[fam]]
F64_STATS_L = O.STATS_L + (2047, 2048, 2049, 4100)
F64_STATS_CASES = [(fam, N, L, "scales") for fam, N in F64_FAMILIES for L in F64_STATS_L] + \
                  [(fam, N, 1729, "outlier") for fam, N in F64_FAMILIES]
F64_MASK_CASES = [(fam, N, L) for fam, N in F64_FAMILIES for L in O.MASK_L + (4100,)]
F64_FACTOR_CASES = [(fam, N, k, ac, cond) for fam, N in F64_FAMILIES for k in (1, 2, 8) for ac in (0.0, 0.3)
                    for cond in (1e1, 1e4) if not (N == 256 and k == 8)]
F64_JITTER_CASES = [("f64", 32), ("n_f64", 24), ("n_f64", 100)]
F64_APPLY_CASES = [(fam, N, L, masked) for fam, N in F64_FAMILIES for L in APPLY_L for masked in (False, True)]

MUTANTS = {
    "stats_n": ("pair_one_sided", "diag_sums_missing", "count_missing", "mask_ignored_last_tile"),
    "apply_n": ("pad_channel_not_zeroed", "partial_block_dropped", "t0_not_added"),
    "stats_f64": ("mean_fp32", "centred_fp32"),
    "factor_f64": ("jitter_not_cumulative",),
    "apply_f64": ("T_fp32", "pad_channel_not_zeroed", "partial_block_dropped", "t0_not_added"),
}
