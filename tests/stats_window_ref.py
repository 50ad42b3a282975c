"""Reference, restatement, mutants, metric and case table of the statistics window (vst_cwct_stats_pool; test infrastructure only;
tests/test_stats_window_host.py and tests/test_gpu_stats_window.py).  Imports no GPU code.

pool_ref is the arithmetic of include/vstnet.h ("Statistics window") in numpy, operation for operation and in increasing age:
dtype = float64 is the restatement of what the device computes, dtype = longdouble (64-bit mantissa: asserted below) the truth.
The usable / scan / copy rules are the header's.  Each switch of MUTANTS makes it wrong in one way.

Metric: the statistics metrics of tests/cwct_ops_ref.py (|err_ij| / sqrt(C_ii C_jj), |err_i| / sqrt(C_ii)) with the POOLED C.
Bound: device <= FACTOR x max(e64, 2^-53), e64 = the restatement against the truth at the same inputs: the project's FACTOR 4
for "the same products in another order".  Records under the copy rule are compared as bits.
"""
import ctypes as C
import itertools
import math

import numpy as np

from cwct_ops_ref import rec_len, stats64, stats_err, unpack      # noqa: F401  (tests/ is on the path: cwct_ops_ref puts it there)

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the truth of the statistics window needs a long double of 64 mantissa bits"

FACTOR = 4.0
FLOOR = 2.0 ** -53
MAX_AGES = 8

MUTANTS = {
    "no_mean_shift": "the n_a (mu_a - mu)(mu_a - mu)^T term is missing",
    "divide_by_M": "S / M instead of S / (M - 1)",
    "n_for_n_minus_1": "n_a C_a instead of (n_a - 1) C_a",
    "weights_not_in_M": "M = sum n_a, the weights ignored",
    "scan_past_cut": "the scan drops the age that fails the cut test and goes on to older ones",
    "unusable_stops_scan": "an unusable age ends the scan",
    "cut_without_cov": "the cut distance lacks |C_a - C_0|_F",
    "no_copy_rule": "S = {0} goes through the pooled formula instead of the bit copy",
}


def width_of(length):
    n = int(round((math.sqrt(4 * length - 3) - 1) / 2))
    assert rec_len(n) == length, length
    return n


def cut_distance(rec_a, rec_0, N, dtype=np.longdouble, mut=()):
    """(|mu_a - mu_0|^2 + |C_a - C_0|_F, tr(C_0)) of two records"""
    _, ma, ca = unpack(np.asarray(rec_a).astype(dtype), N)
    _, m0, c0 = unpack(np.asarray(rec_0).astype(dtype), N)
    dm = ((ma - m0) ** 2).sum()
    dc = np.sqrt(((ca - c0) ** 2).sum())
    return (dm if "cut_without_cov" in mut else dm + dc), np.trace(c0)


def pool_ref(records, weights, cut, dtype=np.float64, mut=(), trace=None):
    """records: newest first, each [R, rec] (or [rec]) float64; weights: one per age -> (out [R, rec] in `dtype`, used int [R]).
    trace (a list): every cut decision made is appended as (record, age, distance, limit)."""
    recs = [np.asarray(r, dtype=np.float64).reshape(-1, np.asarray(r).shape[-1]) for r in records]
    R, length = recs[0].shape
    N = width_of(length)
    out = np.empty((R, length), dtype=dtype)
    used = np.zeros(R, dtype=np.int32)
    w = [dtype(x) for x in weights]
    one = dtype(1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(R):
            rows = [a[r].astype(dtype) for a in recs]
            cnt = [row[0] for row in rows]
            usable = [bool(c >= 2.0) for c in cnt]
            out[r] = rows[0]
            if not usable[0]:
                continue
            sel = [0]
            for a in range(1, len(rows)):
                if not usable[a]:
                    if "unusable_stops_scan" in mut:
                        break
                    continue
                if cut > 0:
                    d, tr = cut_distance(rows[a], rows[0], N, dtype, mut)
                    if trace is not None:
                        trace.append((r, a, d, dtype(cut) * tr))
                    if d > dtype(cut) * tr:
                        if "scan_past_cut" in mut:
                            continue
                        break
                sel.append(a)
            used[r] = len(sel)
            if len(sel) == 1 and "no_copy_rule" not in mut:
                continue
            m = [w[a] * cnt[a] for a in sel]
            M = dtype(0.0)
            for a, ma in zip(sel, m):
                M = M + (cnt[a] if "weights_not_in_M" in mut else ma)
            acc = np.zeros(N, dtype=dtype)
            for a, ma in zip(sel, m):
                acc = acc + ma * rows[a][1:1 + N]
            mu = acc / M
            S = np.zeros((N, N), dtype=dtype)
            for a in sel:
                d = rows[a][1:1 + N] - mu
                t = (cnt[a] if "n_for_n_minus_1" in mut else cnt[a] - one) * rows[a][1 + N:].reshape(N, N)
                if "no_mean_shift" not in mut:
                    t = t + (cnt[a] * d)[:, None] * d[None, :]
                S = S + w[a] * t
            out[r, 0], out[r, 1:1 + N] = M, mu
            out[r, 1 + N:] = (S / (M if "divide_by_M" in mut else M - one)).reshape(-1)
    return out, used


def pool_errors(got, truth, used, N):
    """(cov error, mean error) of a pooled block against the truth, the largest over its records: the statistics metric where a
    record was pooled, inf for any differing bit where the copy rule holds (the truth is then the age-0 record itself)"""
    ec = em = 0.0
    got, truth = np.asarray(got), np.asarray(truth)
    for r in range(truth.shape[0]):
        if used[r] <= 1:
            same = np.array_equal(np.asarray(got[r], dtype=np.float64).view(np.uint64),
                                  np.asarray(truth[r], dtype=np.float64).view(np.uint64))
            c = m = 0.0 if same else math.inf
        else:
            c, m = stats_err(np.asarray(got[r]).astype(np.longdouble), truth[r], N)
            cn = abs(float(got[r][0]) - float(truth[r][0])) / abs(float(truth[r][0]))      # the count rides with the mean
            m = max(m, cn)
        ec, em = max(ec, c), max(em, m)
    return ec, em


def pool_ratio(got, r64, truth, used, N):
    """the larger of the covariance and the mean ratio, each against its own e64; <= FACTOR passes"""
    (gc, gm), (ec, em) = pool_errors(got, truth, used, N), pool_errors(r64, truth, used, N)
    with np.errstate(invalid="ignore"):
        return max(gc / max(ec, FLOOR), gm / max(em, FLOOR)), (gc, gm, ec, em)


# ================================================================================================================ the case table
# (N, n_records, n_ages, decay (or a tuple of explicit weights), unusable, prefactored, cut)
#   unusable     "none" | "age0" | "middle" (age 1 of >= 3) | "all_but_0": records with n = 0 and n = 1 (alternating) at those ages,
#                in the even records of the block (record 0 among them); the odd records stay usable throughout
#   prefactored  the record of age 2 has n < 0 (every record of the block)
#   cut          "none" | "age1" (age 1 is another scene by its mean, the older ages are the first scene again: they must stay out)
#                | "age3" (the same at age 3, by the covariance alone) | "age2_behind_unusable" (age 1 unusable, age 2 another scene)
CUT = 2.0            # the table's threshold: same-scene distances sit under CUT / 4 x tr(C_0), other scenes above 4 x CUT x tr(C_0)
WIDTHS = (1, 7, 16, 32, 128, 256)


def _valid(ages, unusable, pref, cut):
    if unusable == "middle" and ages < 3 or unusable == "all_but_0" and ages < 2:
        return False
    if pref and ages < 3:
        return False
    if cut == "age1" and ages < 2 or cut == "age3" and ages < 4 or cut == "age2_behind_unusable" and ages < 3:
        return False
    if cut == "age2_behind_unusable" and unusable not in ("none", "middle"):
        return False
    return True


def _cases():
    combos = [c for c in itertools.product((1, 2, 3, 8), (1.0, 0.5), ("none", "age0", "middle", "all_but_0"), (False, True),
                                           ("none", "age1", "age3", "age2_behind_unusable")) if _valid(c[0], *c[2:])]
    small = [(N, R) for N in (1, 7, 16, 32) for R in (1, 8, 32)]
    out = [small[k % len(small)] + c for k, c in enumerate(combos)]
    for N in (128, 256):                                   # the wide records: a few cases each, every rule among them
        out += [(N, 1, 8, 1.0, "none", False, "none"), (N, 8, 8, 0.5, "middle", True, "age3"),
                (N, 1, 3, 0.5, "none", False, "age2_behind_unusable"), (N, 8, 2, 1.0, "age0", False, "age1"),
                (N, 1, 1, 1.0, "none", False, "none"), (N, 8, 3, 1.0, "all_but_0", False, "none")]
    for N, R in ((7, 8), (32, 1), (128, 8)):               # weights of the caller's own (w_0 != 1): what decay ** age never gives
        out += [(N, R, 3, (0.7, 0.2, 0.1), "all_but_0", False, "none"), (N, R, 3, (0.7, 0.2, 0.1), "none", False, "age1"),
                (N, R, 3, (0.5, 0.25, 0.25), "none", False, "none")]
    return out


CASES = _cases()


def case_id(case):
    N, R, ages, decay, unusable, pref, cut = case
    decay = "w" + "_".join(str(w) for w in decay) if isinstance(decay, tuple) else f"d{decay}"
    return f"N{N}-R{R}-W{ages}-{decay}-{unusable}-{'pref-' if pref else ''}{cut}"


def _layout(case, r):
    """(scene per age, unusable per age) of record r of a case"""
    N, R, ages, decay, unusable, pref, cut = case
    scene = ["A"] * ages
    if cut == "age1":
        scene[1] = "B"
    elif cut == "age3":
        scene[3] = "C"
    elif cut == "age2_behind_unusable":
        scene[2] = "B"
    bad = [(r % 2 == 0 and ((unusable == "age0" and a == 0) or (unusable == "middle" and a == 1)
                            or (unusable == "all_but_0" and a > 0))) or (cut == "age2_behind_unusable" and a == 1)
           for a in range(ages)]
    return scene, bad


def case_input(case):
    """-> (records: n_ages arrays [R, rec] float64, newest first; weights float64 [n_ages]; cut).  Seeded by the case.
    Every record is stats64 of float32 data: per-channel scales over 1e-2 .. 1e2, |mean| / std up to 100, a frame-to-frame drift
    of the means of 0.1 std (so the mean-shift term is real) and a pixel count that differs from age to age."""
    N, R, ages, decay, unusable, pref, cut = case
    rng = np.random.default_rng(7919 * N + 131 * R + 17 * ages + int(np.sum(decay) * 10) + 3 * len(unusable) + len(cut) + pref)
    records = [np.empty((R, rec_len(N))) for _ in range(ages)]
    for r in range(R):
        scene, bad = _layout(case, r)
        scales = rng.permutation(np.logspace(-2, 2, N)) if N > 1 else np.array([3.0])
        mean = rng.uniform(-100.0, 100.0, N) * scales
        for a in range(ages):
            L = (a + r // 2) % 2 if bad[a] else 800 + 37 * a + 5 * r       # (unusable: n = 0 and n = 1, both)
            sc = scales * (8.0 if scene[a] == "C" else 1.0)
            mu = mean + (20.0 * scales if scene[a] == "B" else 0.0) + 0.1 * scales * rng.standard_normal(N)
            x = (mu[:, None] + sc[:, None] * rng.standard_normal((N, L))).astype(np.float32)
            records[a][r] = stats64(x)
            if pref and a == 2:
                records[a][r, 0] = -records[a][r, 0]
    weights = np.array(decay if isinstance(decay, tuple) else [decay ** a for a in range(ages)], dtype=np.float64)
    return records, weights, (0.0 if cut == "none" else CUT)


def expected_used(case):
    """what the rules give for the table's constructions, per record: the test of the table itself"""
    N, R, ages, decay, unusable, pref, cut = case
    out = []
    for r in range(R):
        scene, bad = _layout(case, r)
        n = 0 if bad[0] else 1
        for a in range(1, ages if n else 0):
            if bad[a] or (pref and a == 2):
                continue
            if scene[a] != "A":
                break
            n += 1
        out.append(n)
    return np.array(out, dtype=np.int32)


# ================================================================================================================ the A / B clip
# Two scenes for the drift and cut tests: A = synthetic_frames(seed = 1), B = 0.5 synthetic_frames(seed = 2) + 0.3 (another
# exposure and contrast), both quantised to uint8; noisy_u8 adds N(0, sigma^2) before the quantisation: a near-duplicate frame.
CUT_T = 0.01         # the threshold of the cut tests: tests/test_stats_window_host.py holds near-duplicates under T / 4, A against B over 4 T


def _to_u8(x):
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)


def scenes_u8(H=48, W=64):
    """(A, B) as uint8 [H, W, 3]"""
    from vstnet_amd.synth import synthetic_frames
    a = synthetic_frames(1, H, W, seed=1)[0].numpy().transpose(1, 2, 0)
    b = 0.5 * synthetic_frames(1, H, W, seed=2)[0].numpy().transpose(1, 2, 0) + 0.3
    return _to_u8(a), _to_u8(b)


def noisy_u8(frame_u8, seed, sigma=0.02):
    rng = np.random.default_rng(seed)
    return _to_u8(frame_u8.astype(np.float64) / 255.0 + sigma * rng.standard_normal(frame_u8.shape))


# ============================================================================================================ argument errors
def pool_error_cases(rec0=0x10000, out=0x4000000, N=32, n_records=2):
    """(name, expected status, argument tuple without the stream) of every refusal of vst_cwct_stats_pool; `rec0`, `out` = two
    addresses far enough apart; the host test makes
    the calls on addresses that are never dereferenced, the GPU test on real buffers."""
    vp, dbl = C.c_void_p, C.c_double
    nbytes = n_records * rec_len(N) * 8
    ptrs = lambda *p: (vp * len(p))(*p)                         # noqa: E731
    ws = lambda *w: (dbl * len(w))(*w)                          # noqa: E731
    good_p, good_w = ptrs(rec0, rec0 + nbytes), ws(1.0, 0.5)
    cases = [
        ("records null", -1, (None, good_w, 2, n_records, N, 0.0, vp(out), None)),
        ("weights null", -1, (good_p, None, 2, n_records, N, 0.0, vp(out), None)),
        ("out null", -1, (good_p, good_w, 2, n_records, N, 0.0, None, None)),
        ("a record null", -1, (ptrs(rec0, 0), good_w, 2, n_records, N, 0.0, vp(out), None)),
        ("out misaligned", -1, (good_p, good_w, 2, n_records, N, 0.0, vp(out + 4), None)),
        ("a record misaligned", -1, (ptrs(rec0, rec0 + nbytes + 4), good_w, 2, n_records, N, 0.0, vp(out), None)),
        ("weight zero", -1, (good_p, ws(1.0, 0.0), 2, n_records, N, 0.0, vp(out), None)),
        ("weight negative", -1, (good_p, ws(-1.0, 0.5), 2, n_records, N, 0.0, vp(out), None)),
        ("weight nan", -1, (good_p, ws(1.0, float("nan")), 2, n_records, N, 0.0, vp(out), None)),
        ("weight inf", -1, (good_p, ws(float("inf"), 0.5), 2, n_records, N, 0.0, vp(out), None)),
        ("cut negative", -1, (good_p, good_w, 2, n_records, N, -0.5, vp(out), None)),
        ("cut nan", -1, (good_p, good_w, 2, n_records, N, float("nan"), vp(out), None)),
        ("out is an input", -1, (ptrs(rec0, out), good_w, 2, n_records, N, 0.0, vp(out), None)),
        ("out overlaps an input's end", -1, (ptrs(rec0, out - nbytes + 8), good_w, 2, n_records, N, 0.0, vp(out), None)),
        ("out overlaps an input's start", -1, (ptrs(rec0, out + nbytes - 8), good_w, 2, n_records, N, 0.0, vp(out), None)),
        ("no ages", -2, (good_p, good_w, 0, n_records, N, 0.0, vp(out), None)),
        ("nine ages", -2, (good_p, good_w, 9, n_records, N, 0.0, vp(out), None)),
        ("no records", -2, (good_p, good_w, 2, 0, N, 0.0, vp(out), None)),
        ("33 records", -2, (good_p, good_w, 2, 33, N, 0.0, vp(out), None)),
        ("N = 0", -2, (good_p, good_w, 2, n_records, 0, 0.0, vp(out), None)),
        ("N = 257", -2, (good_p, good_w, 2, n_records, 257, 0.0, vp(out), None)),
    ]
    return cases
