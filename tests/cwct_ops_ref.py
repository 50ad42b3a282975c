"""References, host restatements, mutants, metrics and case tables of the per-kernel cWCT tests (test infrastructure only;
tests/test_cwct_ops_host.py and tests/test_gpu_cwct_ops.py).  Imports no GPU code.

References (fp64): two-pass mean / covariance over all pixels, one label or every slot of a plan; the plan rule of
label_plan_kernel; the factor of include/vstnet.h ("cWCT": Lc, Ls_i, mixL, T = mixL Lc^-1, t0) and y = T x + t0.
Restatements (fp32, one CPU thread): what the device computes, in the device's number formats but not in the matrix cores'
summation order - per-workgroup shifted sums over the groups cwct_stats_groups gives, combined in fp64 by Chan's update; the
fp32 Cholesky with LAPACK's failure rule and the cumulative jitter (its rank-1 update an fma, as fac_chol writes it: with a
smallest eigenvalue of 1.5 eps a product and a subtraction land 7 x away), the mix and the triangular solve; the fp32 apply; the split
apply Th xl + Tl xh + Th xh with the bf16 split of tests/emul.py.  Each has switches that make it wrong in one way (MUTANTS).

Metrics that do not let a large channel hide a small one:
  covariance |err_ij| / sqrt(C_ii C_jj)        mean |err_i| / sqrt(C_ii)
  apply      |err_ip| / (sum_k |T_ik| |x_kp| + |t0_i|)
  factor     |dT_ij| / (|mixL| |Lc^-1|)_ij     t0 |dt0_i| / (|mix_mean_i| + (|mixL| |Lc^-1| |mean_c|)_i)

Bounds: device error <= FACTOR[op] x max(e32, FLOOR[op]), e32 = the restatement against fp64 at the same inputs under the same
metric.  By that definition the restatement itself sits at <= 1 = FACTOR / 4; FACTOR is the room the device gets for summing
the same fp32 products in another order (the matrix cores' trees against the host's BLAS blocks): two fp32 evaluations of one
sum each err by up to e, so they differ from the truth by up to about 2 e32 when their roundings are independent, and 4 leaves
a factor of two on top of that, the figure the segmenter's GEMM and attention tests settled on.  The floor is u: storing the exact
result in fp32 costs that much, so an e32 below u (L = 2, a single product) says nothing.  Every mutant must exceed
1.25 x FACTOR at one case of the tables (tests/test_cwct_ops_host.py asserts it and prints the figures).  The split forms are
measured against the emulated split: their e32 is the emulated split's error, which the host test also holds under the header's
own claim, SPLIT_CLAIM.
"""
import contextlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

U = 2.0 ** -24
EPS = 2e-5                    # the jitter step of cholesky_dec (models/cWCT.py:111-132)
MAX_SLOTS = 32
SPLIT_CLAIM = 1.5e-5          # include/vstnet.h, vst_cwct_apply_prec: "~1.5e-5 max-rel"
OPS = ("stats", "factor", "apply", "apply_split")
FACTOR = {op: 4.0 for op in OPS}
FLOOR = {op: U for op in OPS}
KRES = {32: 8, 64: 4, 128: 1}     # csrc/cwct.hip LabelCfg: slots per statistics pass
KAPP = {32: 8, 64: 4, 128: 1}     # ... and per apply pass
SENTINEL_F32 = np.array([0x7FC0BEEF], dtype=np.uint32).view(np.float32)[0]    # a NaN with a payload: compared as bits
SENTINEL_F64 = -12345.678


def ratio(op, err, e32):
    return err / max(e32, FLOOR[op])


@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def rec_len(n):
    return 1 + n + n * n


def unpack(rec, n):
    """{n, mean, cov} views of a record"""
    rec = np.asarray(rec)
    return float(rec[0]), rec[1:1 + n], rec[1 + n:].reshape(n, n)


def pack(cnt, mean, cov):
    return np.concatenate([[cnt], np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64).reshape(-1)])


# ================================================================================================== launch conditions
# Restated from csrc/cwct.hip; a host test derives from every case which form the launcher takes and asserts that the tables
# reach all of them.  `off` arguments are ELEMENT offsets from a 256-byte aligned allocation (floats: 4 bytes, masks: 1 byte).
def stats_groups(L):
    """cwct_stats_groups (cwct.hip:26-33): (workgroups, pixels per workgroup, regime)"""
    per = 2048
    while per > 512 and L // per < 256:
        per >>= 1
    g = (L + per - 1) // per
    regime = str(per)
    if g > 1024:
        g = 1024
        per = ((L + g - 1) // g + 63) // 64 * 64
        g = (L + per - 1) // per
        regime = "capped"
    return g, per, regime


def stats_form(N, L, x_off, mask_off=None):
    """vst_cwct_stats (cwct.hip:2206-2235)"""
    if N == 16:
        return "fma16"
    vec = L % 4 == 0 and (4 * x_off) % 16 == 0 and (mask_off is None or mask_off % 4 == 0)
    return "mfma_vec" if vec else "mfma_scalar"


def apply_form(N, L, x_off, y_off, masked, precision):
    """launch_apply (cwct.hip:853-873)"""
    al = lambda b: (4 * x_off) % b == 0 and (4 * y_off) % b == 0      # noqa: E731
    if precision != "fp32" and N >= 64 and not masked and L % 64 == 0 and al(16):
        return "split"
    if N >= 32:
        pxm = {32: 4, 64: 2, 128: 1}[N]
        if L % pxm == 0 and L >= pxm and al(4 * pxm):
            return f"mfma{pxm}"
    pxv = 4 if N <= 32 else (2 if N <= 64 else 1)
    return "fma_vec" if pxv > 1 and L % pxv == 0 and al(4 * pxv) else "fma_scalar"


def apply_labels_form(N, L, x_off, y_off, mask_off, precision, max_slots):
    """vst_cwct_apply_labels (cwct.hip:2413-2441): (form, passes)"""
    al = lambda b: (4 * x_off) % b == 0 and (4 * y_off) % b == 0      # noqa: E731
    passes = -(-(max_slots or MAX_SLOTS) // KAPP[N])
    if precision != "fp32" and L % 64 == 0 and al(16) and mask_off % 4 == 0:
        return "split", passes
    if N == 32:
        return ("v4" if L % 4 == 0 and al(16) else "v1"), passes
    return ("v2" if L % 2 == 0 and al(8) else "v1"), passes


def stats_labels_passes(N, max_slots):
    """stats_labels (cwct.hip:1320-1334)"""
    return -(-(max_slots or MAX_SLOTS) // KRES[N])


def code_groups(H, W, sp_steps):
    """stats_code_rect (cwct.hip:2464-2491): (rows, rows per workgroup)"""
    L = H * W if sp_steps == 2 else H * W // 4
    m = 256 if sp_steps == 2 else 128
    return L, ((L + 255) // 256 + m - 1) // m * m


def labels_code_groups(H, W):
    """stats_labels_code_rect (cwct.hip:2566-2587)"""
    L = H * W
    return L, ((L + 511) // 512 + 2047) // 2048 * 2048


def stats_code_form(H, W, sp_steps, rect):
    full = rect is None or tuple(rect) == (0, 0, H, W)
    return ("pm" if sp_steps == 2 else "pm128") + ("" if full else "_rect")


def row_pixels(H, W, sp_steps):
    """(y, x) of every row of a packed code, in the code's own pixel grid (mask_to_code_kernel / row_in_rect, cwct.hip:1392-1408,
    1846-1857): sp_steps 2: image pixels; sp_steps 1: pixels of the H/2 x W/2 code."""
    hq, wq = H // 4, W // 4
    per_cell = 8 if sp_steps == 2 else 2
    r = np.arange(2 * hq * wq * per_cell)
    i = (r >= hq * wq * per_cell).astype(np.int64)
    rr = r - i * hq * wq * per_cell
    cell, g = rr // per_cell, rr % per_cell
    h, w = cell // wq, cell % wq
    if sp_steps == 2:
        return 4 * h + 2 * i + ((g >> 1) & 1), 4 * w + 2 * (g >> 2) + (g & 1)
    return 2 * h + i, 2 * w + g


# ======================================================================================================== statistics
def stats64(x, sel=None):
    """two-pass fp64 record of the columns of x [N, L] (float32 tensor) that `sel` (bool [L]) picks"""
    x = np.asarray(x)
    cols = x if sel is None else x[:, sel]
    cols = cols.astype(np.float64)
    n = cols.shape[1]
    mean = cols.mean(1) if n else np.zeros(x.shape[0])
    d = cols - mean[:, None]
    return pack(n, mean, d @ d.T / (n - 1.0) if n > 1 else np.full((x.shape[0],) * 2, np.nan))


def stats64_chunked(x, chunk=1 << 18):
    """stats64 of all columns of a long x without an fp64 copy of it: two passes over chunks"""
    N, L = x.shape
    s = np.zeros(N)
    for a in range(0, L, chunk):
        s += x[:, a:a + chunk].astype(np.float64).sum(1)
    mean = s / L
    m2 = np.zeros((N, N))
    for a in range(0, L, chunk):
        d = x[:, a:a + chunk].astype(np.float64) - mean[:, None]
        m2 += d @ d.T
    return pack(L, mean, m2 / (L - 1.0))


def plan_ref(cmask, smask):
    """label_plan_kernel (cwct.hip:892-911): (lut [256] with 255 = no slot, slot_label list, overflow)"""
    hc, hs = np.bincount(np.asarray(cmask).reshape(-1), minlength=256), np.bincount(np.asarray(smask).reshape(-1), minlength=256)
    lut, labels, over = np.full(256, 255, dtype=np.uint8), [], 0
    for k in range(256):
        a, b = int(hc[k]), int(hs[k])
        if a > 10 and b > 10 and a / b < 100.0 and b / a < 100.0:
            if len(labels) < MAX_SLOTS:
                lut[k] = len(labels)
                labels.append(k)
            else:
                over = 1
    return lut, labels, over


def _group_record(xg, sel, mut, first_outer=None):
    """fp32 record of one workgroup: (n, shift, sum(x - shift), sum (x - shift)(x - shift)^T) over the columns `sel` picks"""
    shift = xg[:, 0].copy()
    d = (xg[:, sel] - shift[:, None]).astype(np.float32)
    n = d.shape[1]
    asum = d.sum(1, dtype=np.float32)
    dt = torch.from_numpy(np.ascontiguousarray(d))
    q = (dt @ dt.t()).numpy()
    return float(n), shift, asum, q


def combine(records, N, mut=()):
    """cwct_stats_mean_kernel + cwct_stats_cov_kernel (cwct.hip:269-327) in fp64"""
    recs = list(records)
    if "record_dropped" in mut and len(recs) > 1:
        recs = recs[:-1]
    nt = sum(r[0] for r in recs)
    if "count_off_by_one" in mut:
        nt += 1.0
    acc = np.zeros(N)
    for n, sh, a, _ in recs:
        acc += n * sh.astype(np.float64) + a.astype(np.float64)
    mean = acc / nt if nt > 0 else np.zeros(N)
    m2 = np.zeros((N, N))
    for n, sh, a, q in recs:
        if n <= 0:
            continue
        a64 = a.astype(np.float64)
        di = a64 / n - mean if "no_shift_in_combine" in mut else sh.astype(np.float64) + a64 / n - mean
        m2 += q.astype(np.float64) - np.outer(a64, a64) / n + n * np.outer(di, di)
    with np.errstate(divide="ignore", invalid="ignore"):
        return pack(nt, mean, m2 / (nt - 1.0))


def _select(mask_g, label, mut, vec):
    if mask_g is None:
        return None
    sel = mask_g == label
    if "mask_bits_reversed" in mut and vec:
        k = len(sel) // 4 * 4
        sel = sel.copy()
        sel[:k] = sel[:k].reshape(-1, 4)[:, ::-1].reshape(-1)
    return sel


def stats32(x, mask=None, label=0, mut=(), groups=None, vec=True):
    """restatement of vst_cwct_stats on x [N, L] float32"""
    get = lambda a, b: x[:, a:b]      # noqa: E731
    N, L = x.shape
    g, per, _ = groups or stats_groups(L)
    with one_thread():
        recs = []
        for w in range(g):
            a, b = w * per, min((w + 1) * per, L)
            if "last_tile_dropped" in mut and (b - a) % 64:
                b = a + (b - a) // 64 * 64
                if b == a:
                    recs.append((0.0, get(a, a + 1)[:, 0].copy(), np.zeros(N, np.float32), np.zeros((N, N), np.float32)))
                    continue
            xg = get(a, b)
            sel = _select(None if mask is None else mask[a:b], label, mut, vec)
            recs.append(_group_record(xg, slice(None) if sel is None else sel, mut))
    return combine(recs, N, mut)


def stats_labels64(x, mask, lut, n_slots):
    out = np.full((MAX_SLOTS, rec_len(x.shape[0])), SENTINEL_F64)
    sl = lut[mask]
    for s in range(n_slots):
        out[s] = stats64(x, sl == s)
    return out


def stats_labels32(x, mask, lut, n_slots, max_slots=0, mut=(), groups=None):
    """restatement of stats_labels / stats_labels_code_rect: per workgroup and slot the record of that slot's pixels; records of
    slots >= n_slots, or past the passes max_slots covers, keep SENTINEL_F64"""
    N, L = x.shape
    g, per, _ = groups or stats_groups(L)
    kres = KRES[N]
    covered = min(n_slots, -(-(max_slots or MAX_SLOTS) // kres) * kres)
    out = np.full((MAX_SLOTS, rec_len(N)), SENTINEL_F64)
    sl = lut[mask]
    with one_thread():
        for s in range(covered):
            recs = []
            for w in range(g):
                a, b = w * per, min((w + 1) * per, L)
                xg, sg = x[:, a:b], sl[a:b]
                n, sh, asum, q = _group_record(xg, sg == s, mut)
                if "padding_not_zeroed" in mut:
                    # a run whose length is not a multiple of 4 leaves up to 3 stale columns in the tile buffer: what the
                    # previous tile staged there.  The row sums skip them (j < nc); the MFMAs take whole groups of 4.
                    for t0 in range(64, b - a, 64):
                        nc = int((sg[t0:t0 + 64] == s).sum())
                        pad = -nc % 4
                        if nc and pad:
                            stale = (xg[:, t0 - 64 + nc:t0 - 64 + nc + pad] - sh[:, None]).astype(np.float32)
                            q = q + stale @ stale.T
                recs.append((n, sh, asum, q))
            out[s] = combine(recs, N, mut)
    if "second_pass_to_first" in mut:
        for s in range(kres, covered):
            out[s - kres] = out[s]
            out[s] = SENTINEL_F64
    return out


def stats_err(got, want, N, skip=()):
    """(covariance error, mean error) of a record under the normalised metrics; channels in `skip` (constant: C_ii = 0) are left
    to the exact assertions"""
    _, gm, gc = unpack(got, N)
    _, wm, wc = unpack(want, N)
    keep = np.array([c not in skip for c in range(N)])
    sd = np.sqrt(np.diag(wc)[keep])
    ec = np.abs(gc - wc)[np.ix_(keep, keep)] / np.outer(sd, sd)
    em = np.abs(gm - wm)[keep] / sd
    ec, em = np.nan_to_num(ec, nan=np.inf), np.nan_to_num(em, nan=np.inf)
    return float(ec.max()), float(em.max())


def stats_ratio(got, r32, want, N, skip=()):
    """the larger of the covariance and the mean ratio, each against its own e32"""
    (gc, gm), (ec, em) = stats_err(got, want, N, skip), stats_err(r32, want, N, skip)
    return max(ratio("stats", gc, ec), ratio("stats", gm, em)), (gc, gm, ec, em)


# ---- inputs
CONST_CH, CONST_VAL = 2, 50.25


def stats_input(N, L, kind="scales", seed=0):
    """[N, L] float32: channel deviations from 0.01 to 3 around an offset of 50 (the existing test's), channel 1 nearly collinear
    with channel 0, channel CONST_CH constant; kind "outlier": the first pixel of every workgroup is 1e4 (the worst shift)"""
    g = torch.Generator().manual_seed(1000 * N + L % 100003 + 7 * seed)
    scales = torch.logspace(-2, math.log10(3.0), N, dtype=torch.float64)
    z = torch.randn(N, L, generator=g, dtype=torch.float64)
    z[1] = z[0] + 1e-3 * z[1]
    x = (50.0 + scales[:, None] * z).float()
    x[CONST_CH] = CONST_VAL
    if kind == "outlier":
        _, per, _ = stats_groups(L)
        x[:, ::per] = 1e4
        x[CONST_CH] = CONST_VAL
    return x.numpy()


def long_input(L):
    """the N = 32 input of a long case, made chunk by chunk (float32 throughout: 128 L bytes)"""
    scales = torch.logspace(-2, math.log10(3.0), 32, dtype=torch.float32)[:, None]
    x = np.empty((32, L), dtype=np.float32)
    ch = 1 << 18
    for k in range(-(-L // ch)):
        a, b = k * ch, min((k + 1) * ch, L)
        g = torch.Generator().manual_seed(77 + k)
        x[:, a:b] = (50.0 + scales * torch.randn(32, b - a, generator=g, dtype=torch.float32)).numpy()
    x[CONST_CH] = CONST_VAL
    return x


STATS_N = (16, 32, 64, 128)
STATS_L = (2, 63, 64, 65, 68, 132, 192, 516, 1729)
STATS_LONG = (262144 + 68, 524288 + 68, 2097152 + 68)
STATS_CASES = [(N, L, off, "scales") for N in STATS_N for L in STATS_L for off in (0, 1)] + \
              [(N, 1729, 0, "outlier") for N in STATS_N]
MASK_L = (68, 516, 1729)
MASK_LABELS = (0, 255, 7)
MASK_CASES = [(N, L, moff, lab) for N in STATS_N for L in MASK_L for moff in (0, 1) for lab in MASK_LABELS]


def one_label_mask(L):
    """labels 0, 255 and 7: 7 at exactly 2 pixels; 0 absent from the tiles 64..127 and 192..255 and (L >= 516) from the whole
    second workgroup, pixels 512..1023; 255 absent from the third tile"""
    g = np.random.RandomState(L)
    m = np.where(g.rand(L) < 0.5, 0, 255).astype(np.uint8)
    m[64:128] = 255
    m[192:256] = 255
    m[128:192] = 0
    m[512:1024] = 255
    m[[3, L - 1]] = 7
    return m[:L]


# ---- plans
def plan_labels(n):
    """n slot labels in increasing order, 0 and 255 among them when n > 1"""
    return [0] if n == 1 else sorted({int(round(v)) for v in np.linspace(0, 255, n)})


PLAN_KINDS = ("tile", "round_robin", "runs", "slotless", "absent")


def plan_mask(L, n, kind, N=32):
    """(content mask [L], style mask) with exactly n valid labels"""
    labs = np.array(plan_labels(n), dtype=np.uint8)
    p = np.arange(L)
    if kind == "tile":
        m = labs[(p // 64) % n]                       # whole 64-pixel tiles of one slot
    elif kind in ("round_robin", "slotless", "absent"):
        m = labs[p % n]
    elif kind == "runs":                              # runs of 1, 2, 3 and 5 pixels in a cycle of 7 (coprime with every slot count
        runs = np.resize(np.array([1, 2, 3, 5, 1, 3, 2]), L)      # used): every slot meets every remainder of 4 in some tile
        ids = np.repeat(np.arange(L), runs)[:L]
        m = labs[ids % n]
    else:
        raise ValueError(kind)
    m = m.copy()
    free = [v for v in range(1, 255) if v not in set(labs.tolist())]
    extra_s = []
    if kind == "slotless":
        m[5::97][:5] = free[0]                        # 5 pixels: count <= 10
        m[11::89][:11] = free[1]                      # 11 pixels against 1100 style pixels: ratio >= 100
        extra_s = [np.full(1100, free[1], dtype=np.uint8), np.full(40, free[0], dtype=np.uint8)]
    if kind == "absent" and n > 1:
        _, per, _ = stats_groups(L)
        keep = m[per:] == labs[0]
        m[per:][keep] = labs[1]                       # slot 0 lives in the first workgroup only
    smask = np.concatenate([m] + extra_s)
    return m, smask


def plan_cases(N):
    k = KRES[N]
    counts = [(1, 0, "tile"), (1, 1, "runs"), (k, 0, "round_robin"), (k, k, "runs"), (k + 1, 0, "runs"),
              (k + 1, k + 1, "absent"), (32, 0, "round_robin"), (32, 32, "slotless"), (k + 1, 0, "slotless"), (32, 32, "runs")]
    out = []
    for c in counts:
        if c not in out:
            out.append(c)
    return out


PLAN_L = (1092, 1729)
PLAN_CASES = [(N, L) + c for N in (32, 64, 128) for L in PLAN_L for c in plan_cases(N)]


def plan_input(N, L):
    return stats_input(N, L, "scales", seed=3)


# ---- packed rows
CODE_CASES = [   # (sp_steps, H, W, rect or None)
    (2, 8, 8, None), (2, 8, 8, (1, 2, 5, 3)), (2, 24, 40, None), (2, 24, 40, (3, 5, 17, 22)), (2, 24, 40, (0, 7, 24, 1)),
    (2, 24, 40, (11, 0, 1, 40)), (2, 72, 104, None), (2, 72, 104, (10, 6, 50, 91)),
    (1, 16, 16, None), (1, 16, 16, (2, 6, 10, 8)), (1, 48, 80, None), (1, 48, 80, (6, 10, 30, 52)), (1, 48, 80, (0, 2, 48, 2)),
    (1, 48, 80, (4, 0, 2, 80)),
]
CODE_LABEL_CASES = [(24, 40, 3, None), (24, 40, 3, (3, 5, 17, 22)), (72, 104, 9, None), (72, 104, 9, (10, 6, 50, 91)),
                    (72, 104, 9, (0, 7, 72, 1))]


def code_input(sp_steps, H, W):
    """z of an H x W image: [32, H, W] or [128, H/2, W/2]"""
    N, h, w = (32, H, W) if sp_steps == 2 else (128, H // 2, W // 2)
    return stats_input(N, h * w, "scales", seed=11).reshape(N, h, w)


def code_rows(z, H, W, sp_steps):
    """the rows of z's packed code, [rows, N], in the code's order (what vst_z_to_code writes, one row per code pixel)"""
    y, x = row_pixels(H, W, sp_steps)
    return np.ascontiguousarray(z[:, y, x].T)


def rect_rows(H, W, sp_steps, rect):
    """bool per row: its pixel lies in the rectangle (image pixels; artistic rows are 2 x 2 pixels)"""
    y, x = row_pixels(H, W, sp_steps)
    if rect is None:
        return np.ones(len(y), dtype=bool)
    f = 2 if sp_steps == 1 else 1
    y0, x0, h, w = rect
    return (y >= y0 // f) & (y < (y0 + h) // f) & (x >= x0 // f) & (x < (x0 + w) // f)


def code_label_mask(H, W, n):
    """[H, W] uint8 with n valid labels in blobs that cut the cells, and a sprinkle of a slotless label"""
    labs = np.array(plan_labels(n), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    m = labs[((yy * 3 + xx * 5) // 7) % n].copy()
    free = [v for v in range(1, 255) if v not in set(labs.tolist())][0]
    m.reshape(-1)[3::101][:6] = free
    return m


# ============================================================================================================ factor
def chol32(a, fused=True):
    """right-looking fp32 Cholesky with LAPACK's failure rule (fac_chol, cwct.hip:377-439): (L, failed, pivots d_j met so far)"""
    a = a.astype(np.float32).copy()
    n = a.shape[0]
    piv = []
    for j in range(n):
        d = a[j, j]
        piv.append(float(d))
        if not d > 0:
            return None, True, piv
        p = np.sqrt(d, dtype=np.float32)
        rp = np.float32(1.0) / p
        col = (a[j + 1:, j] * rp).astype(np.float32)
        a[j, j] = p
        a[j + 1:, j] = col
        c64 = col.astype(np.float64)                       # the update is an fma on the device: one rounding of a - col col^T
        a[j + 1:, j + 1:] = (a[j + 1:, j + 1:].astype(np.float64) - np.outer(c64, c64)).astype(np.float32) if fused else \
            a[j + 1:, j + 1:] - np.outer(col, col).astype(np.float32)
    return np.tril(a), False, piv


def jittered(cov, tries, eps, mut=()):
    """fac_load (cwct.hip:358-372): float(cov) + eps, + 2 eps, ... on the diagonal, every addition rounded to fp32"""
    a = cov.astype(np.float32).copy()
    d = np.diag(a).copy()
    ts = range(1, tries + 1) if "jitter_not_cumulative" not in mut else ([tries] if tries else [])
    for t in ts:
        d = (d + np.float32(float(t) * float(np.float32(eps)))).astype(np.float32)
    a[np.diag_indices_from(a)] = d
    return a


def factor_chol32(rec, N, eps, min_tries=0, mut=(), trace=None):
    """fac_factor (cwct.hip:444-463): (L fp32, tries)"""
    cnt, _, cov = unpack(rec, N)
    if cnt < 0:
        return cov.astype(np.float32), 0
    tries = max(0, min_tries)
    last_fail = None
    while True:
        L, failed, piv = chol32(jittered(cov, tries, eps, mut))
        if not failed:
            break
        last_fail = piv[-1]
        tries += 1
    if trace is not None:
        trace.append({"tries": tries, "last_failed_pivot": last_fail, "min_pivot": min(piv),
                      "diag": float(np.abs(np.diag(cov)).max())})
    return L, tries


def factor32(content, styles, alphas, alpha_c, N, eps=EPS, min_tries=None, mut=(), trace=None):
    """restatement of cwct_factor_kernel (cwct.hip:465-586): (affine float32 [N*N + N], info [2 + n_styles])"""
    k = len(styles)
    mt = list(min_tries) if min_tries is not None else [0] * (2 + k)
    styles, alphas = list(styles), list(alphas)
    if "style_dropped" in mut and k > 1:
        styles, alphas = styles[:-1], alphas[:-1]
    m = np.zeros((N, N), np.float32)
    mixmu = np.zeros(N)
    info = [0] * (2 + k)
    for s, (rec, al) in enumerate(zip(styles, alphas)):
        r, info[2 + s] = factor_chol32(rec, N, eps, mt[2 + s], mut, trace)
        al = np.float32(al)
        mixmu += unpack(rec, N)[1].astype(np.float32).astype(np.float64) * float(al)
        m = (m + r * al).astype(np.float32)
    Lc, info[0] = factor_chol32(content, N, eps, mt[0], mut, trace)
    _, cmean, _ = unpack(content, N)
    if alpha_c != 0.0 and "alpha_c_dropped" not in mut:
        ac = np.float32(alpha_c)
        mixmu = mixmu * float(np.float32(1.0) - ac) + cmean.astype(np.float32).astype(np.float64) * float(ac)
        m = ((m * (np.float32(1.0) - ac)).astype(np.float32) + (Lc * ac).astype(np.float32)).astype(np.float32)
    for j in range(N - 1, -1, -1):                              # T Lc = mixL, last column first
        t = (m[:, j] * (np.float32(1.0) / Lc[j, j])).astype(np.float32)
        m[:, j] = t
        m[:, :j] -= np.outer(t, Lc[j, :j]).astype(np.float32)
    mc = cmean if "t0_mean_unrotated" not in mut else None
    t0 = mixmu - (m.astype(np.float64) @ cmean if mc is not None else cmean)
    return np.concatenate([m.reshape(-1), t0.astype(np.float32)]), info


def factor64(content, styles, alphas, alpha_c, N, tries, eps=EPS):
    """the factor in fp64 with the jitter the given retry counts add ({content, flag, styles...}): (T, t0, denominators)"""
    def chol(rec, t):
        cnt, _, cov = unpack(rec, N)
        if cnt < 0:
            return cov.copy()
        return np.linalg.cholesky(cov + np.eye(N) * (float(np.float32(eps)) * t * (t + 1) / 2.0))
    mixL, mixmu = np.zeros((N, N)), np.zeros(N)
    for s, (rec, al) in enumerate(zip(styles, alphas)):
        al = float(np.float32(al))
        mixL += chol(rec, tries[2 + s]) * al
        mixmu += unpack(rec, N)[1] * al
    Lc = chol(content, tries[0])
    cmean = unpack(content, N)[1]
    if alpha_c != 0.0:
        ac = float(np.float32(alpha_c))
        mixL = mixL * (1.0 - ac) + Lc * ac
        mixmu = mixmu * (1.0 - ac) + cmean * ac
    Li = np.linalg.inv(Lc)
    T = mixL @ Li
    dT = np.abs(mixL) @ np.abs(Li)
    return T, mixmu - T @ cmean, dT, np.abs(mixmu) + dT @ np.abs(cmean)


def factor_err(aff, ref, N):
    T, t0, dT, dt0 = ref
    aff = np.asarray(aff, dtype=np.float64)
    gT, g0 = aff[:N * N].reshape(N, N), aff[N * N:]
    low = np.tril(np.ones((N, N), dtype=bool))
    eT = np.where(low, np.abs(gT - T) / np.where(dT > 0, dT, 1.0), np.where(gT == 0, 0.0, np.inf))
    return max(float(eT.max()), float((np.abs(g0 - t0) / dt0).max()))


def spd(N, cond, seed, scale=1.0):
    """fp64 covariance record material: Q diag(lambda) Q^T with eigenvalues log-spaced over `cond`"""
    g = np.random.RandomState(seed)
    q, _ = np.linalg.qr(g.randn(N, N))
    lam = scale * np.logspace(0, -math.log10(cond), N)
    c = (q * lam) @ q.T
    return (c + c.T) / 2


def record(N, cov, seed, n=4096.0):
    return pack(n, np.random.RandomState(seed + 99).randn(N) * 2.0 + 1.0, cov)


FACTOR_CASES = [(N, k, ac, cond) for N in STATS_N for k in (1, 2, 8) for ac in (0.0, 0.3) for cond in (1e1, 1e4)]
JITTER_KINDS = ("rank_deficient", "constant_channel", "indefinite")


def factor_input(N, k, cond, seed=0):
    content = record(N, spd(N, cond, 10 * N + seed), seed)
    styles = [record(N, spd(N, 30.0, 10 * N + 100 + s + seed, scale=0.5 + 0.25 * s), 200 + s + seed) for s in range(k)]
    al = np.linspace(1.0, 2.0, k)
    return content, styles, (al / al.sum()).tolist()


def jitter_content(N, kind):
    """content records that need the jitter.  The retry count must not hang on a rounding, so each is built in fp64 with its
    smallest eigenvalue a known multiple of EPS below zero (or a pivot that is exactly zero):
      rank_deficient   : N - 4 pixels (fewer than channels) give N - 4 - 1 non-zero eigenvalues; 1.5 EPS is taken off the diagonal,
                         so the null space sits at -1.5 EPS: try 0 and try 1 (+ EPS) fail, try 2 (+ 3 EPS) leaves + 1.5 EPS
      constant_channel : a zero row and column: the pivot is exactly 0 at try 0 (0 > 0 fails whatever the rounding), EPS at try 1
      indefinite       : well-conditioned with one eigenvalue at -4.5 EPS: tries 0, 1, 2 fail, try 3 (+ 6 EPS) leaves 1.5 EPS"""
    g = np.random.RandomState(5 * N + len(kind))
    if kind == "rank_deficient":
        x = g.randn(N, N - 4)
        d = x - x.mean(1, keepdims=True)
        cov = d @ d.T / (N - 5.0) - 1.5 * EPS * np.eye(N)
    elif kind == "constant_channel":
        cov = spd(N, 10.0, 3 * N)
        cov[CONST_CH, :] = 0.0
        cov[:, CONST_CH] = 0.0
    else:
        q, _ = np.linalg.qr(g.randn(N, N))
        lam = np.linspace(0.5, 2.0, N)
        lam[0] = -4.5 * EPS
        cov = (q * lam) @ q.T
        cov = (cov + cov.T) / 2
    return record(N, cov, 17)


# ============================================================================================================= apply
def apply64(x, aff, N):
    aff = np.asarray(aff, dtype=np.float64)
    T, t0 = aff[:N * N].reshape(N, N), aff[N * N:]
    x = np.asarray(x, dtype=np.float64)
    return T @ x + t0[:, None], np.abs(T) @ np.abs(x) + np.abs(t0)[:, None]


def apply32(x, aff, N, mut=()):
    """restatement of the fp32 apply kernels"""
    T, t0 = aff[:N * N].reshape(N, N), aff[N * N:]
    with one_thread():
        y = (torch.from_numpy(np.ascontiguousarray(T)) @ torch.from_numpy(np.ascontiguousarray(x))).numpy()
    if "t0_not_added" not in mut:
        y = y + t0[:, None]
    return _skip_last(y.astype(np.float32), x, mut)


def _bf16_split(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi.numpy(), lo.numpy()


def apply_split32(x, aff, N, mut=()):
    """restatement of cwct_apply_split_kernel (cwct.hip:745-817): Th xl + Tl xh + Th xh, products exact, fp32 accumulation"""
    T, t0 = aff[:N * N].reshape(N, N), aff[N * N:]
    th, tl = _bf16_split(T)
    xh, xl = _bf16_split(x)
    prods = [(th, xl), (tl, xh), (th, xh)]
    if "split_product_missing" in mut:
        prods = prods[1:]
    with one_thread():
        y = sum((torch.from_numpy(a) @ torch.from_numpy(b)) for a, b in prods).numpy()
    if "t0_not_added" not in mut:
        y = y + t0[:, None]
    return _skip_last(y.astype(np.float32), x, mut)


def _skip_last(y, x, mut, group=32):
    if "last_group_skipped" in mut:
        L = y.shape[1]
        a = (L - 1) // group * group
        y = y.copy()
        y[:, a:] = SENTINEL_F32
    return y


def apply_err(got, want, den):
    e = np.abs(np.asarray(got, dtype=np.float64) - want) / den
    return float(np.nan_to_num(e, nan=np.inf).max())


def apply_labels_ref(x, affines, mask, lut, n_slots, N, fn, max_slots=0, mut=()):
    """per-slot maps by `fn` (apply64 / apply32 / apply_split32 on the slot's pixels); pixels without a slot keep x.  The passes
    are restated for their mutants: pass i covers slots [i KAPP, (i + 1) KAPP); the first also copies every other pixel."""
    k = KAPP[N]
    covered = min(n_slots, -(-(max_slots or MAX_SLOTS) // k) * k)
    sl = lut[mask]
    out = np.full(x.shape, SENTINEL_F32, dtype=np.float64 if fn is apply64 else np.float32)
    den = np.ones(x.shape)
    for p0 in range(0, max(covered, 1), k):
        mine = (sl >= p0) & (sl < min(p0 + k, covered))
        if p0 == 0 and "first_pass_no_copy" not in mut:
            out[:, ~mine] = x[:, ~mine]
        if p0 > 0 and "later_pass_overwrites" in mut:
            out[:, ~mine] = x[:, ~mine]
        for s in range(p0, min(p0 + k, covered)):
            px = sl == s
            if not px.any():
                continue
            if fn is apply64:
                out[:, px], den[:, px] = apply64(x[:, px], affines[s], N)
            else:
                out[:, px] = fn(x[:, px], affines[s], N)
    return (out, den) if fn is apply64 else out


APPLY_L = (1, 3, 62, 64, 66, 128, 260)
APPLY_OFFS = (0, 1, 2, 4)
APPLY_CASES = [(N, L, prec, masked) for N in STATS_N for L in APPLY_L + ((4096 + 64,) if N == 128 else ())
               for prec in ("fp32", "bf16x3") for masked in (False, True)]
APPLY_LABEL = 9
ZERO_ROW, ZERO_PIXEL = 1, 0


def apply_input(N, L, seed=0):
    """x [N, L] with a zero pixel; affine with |T| over four decades and a zero row"""
    g = np.random.RandomState(31 * N + L % 9973 + seed)
    x = (g.randn(N, L) * np.logspace(-1, 1, N)[:, None]).astype(np.float32)
    x[:, ZERO_PIXEL] = 0.0
    T = g.randn(N, N) * 10.0 ** g.uniform(-3, 1, (N, N))
    T[ZERO_ROW] = 0.0
    t0 = g.randn(N) * 3.0
    return x, np.concatenate([T.reshape(-1), t0]).astype(np.float32)


def apply_mask(L):
    m = np.where(np.random.RandomState(L + 1).rand(L) < 0.6, APPLY_LABEL, 200).astype(np.uint8)
    m[ZERO_PIXEL] = APPLY_LABEL
    if L > 64:
        m[32:64] = 200                                 # a whole wave's pixel group of another label
    return m


def affines_input(N, n_slots, seed=0):
    out = np.full((MAX_SLOTS, N * N + N), SENTINEL_F32, dtype=np.float32)
    for s in range(n_slots):
        out[s] = apply_input(N, 4, seed=100 + s + seed)[1]
    return out


APPLY_LABELS_L = (1088, 1092)
APPLY_LABELS_CASES = [(N, L, prec) + c for N in (32, 64, 128) for L in APPLY_LABELS_L for prec in ("fp32", "bf16x3")
                      for c in plan_cases(N)]

# ------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = {
    "stats": ("last_tile_dropped", "count_off_by_one", "record_dropped", "no_shift_in_combine", "mask_bits_reversed"),
    "stats_labels": ("padding_not_zeroed", "second_pass_to_first"),
    "factor": ("jitter_not_cumulative", "t0_mean_unrotated", "alpha_c_dropped", "style_dropped"),
    "apply": ("t0_not_added", "last_group_skipped"),
    "apply_split": ("split_product_missing",),
    "apply_labels": ("first_pass_no_copy", "later_pass_overwrites"),
}
