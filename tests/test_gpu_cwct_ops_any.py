"""The kernels of csrc/cwct_any.hip (the fp32 `_n` family, N = 1..256) and csrc/cwct64.hip (the `use_double` route: `_f64` and
`_n_f64`) one by one, through vstnet_amd.cwct.ops, against wider references computed on the CPU at test time
(tests/cwct_any_ref.py), at the widths, lengths, pointer offsets and masks at which the launchers pick each kernel form
(tests/test_cwct_any_host.py proves that the tables reach every form and that every mutant of the restatements is caught).

Bounds.  fp32 `_n`: the references, restatements, metrics and bound of tests/test_gpu_cwct_ops.py, unchanged: device error <=
4 x max(e32, u).  fp64: reference in np.longdouble, restatement e64 in float64; statistics and factor <= 4 x max(e64, 2^-53), the
apply |y - y_ref| <= ulp32(y_ref) / 2 + 4 x max(e64, 2^-53) (sum |T||x| + |t0|), every element.  Exact assertions are bitwise:
NaN margins on both sides of every guarded buffer, label counts, the constant channel, a second call into the same buffers, in
place against out of place, masked-out pixels, prefactored against unfactored, retry counts, the give-up flag.  Every test
prints its ratio (-s) before it asserts; DESIGN.md section 5 ("The any-width and fp64 cWCT kernels one by one") has the table.
The module's name makes it run right after tests/test_gpu_cwct_ops.py and not before tests/test_gpu_cwct_any_width.py: the
restatements' one-thread sections (O.one_thread) leave torch's host threading set explicitly, and after that the CPU oracle of
test_transfer_any_width_vs_oracle[160] and [256] failed inside torch.inverse (an MKL error in SLASWP) when this module ran first.

Measured on an MI355X (x max(e, floor), bound 4; 1345 cases, all within it).  fp32 `_n` statistics: reg<4> 1.75 (one label
3.07), reg<8> 1.58 (1.00), reg<16> 1.17 (1.00), tile<2> 2.55 (1.02), tile<4> with 1 / 2 / 3 / 4 channel blocks 2.60 / 2.33 /
2.39 / 2.17 (one label 1.01 / 1.35 / 1.91 / 1.00); the long
cases 0.04 (N = 5, capped groups) and 0.33 / 0.42 / 0.39 (N = 17 at 1024 / 2048 pixels per workgroup / capped).  factor_n 2.18
(N = 3), with jitter 1.01, from a minimum retry count 1.03; prefactored = unfactored bit for bit at every width, so cwctn_chol
stays as it was.  apply_n PG 4 / 2 / 1: 1.64 / 1.47 / 1.19, with a partial column block 1.84 / 1.26 / 1.56.  Next to the tuned
calls at N = 16 .. 128: statistics at most 1.80 (`_n`) and 1.57 (tuned), factor 1.00 both, apply 1.33 both.  fp64 (x max(e64,
2^-53)): stats_f64 2.56 at one chunk, 1.00 / 1.04 at two / three, one label 1.26; stats_n_f64 2.24 (one covariance workgroup per
chunk), 1.49 / 1.77 / 1.15 at gridDim.y = 2 / 10 / 64, one label 1.69; factor_f64 1.79 (jitter 1.10), factor_n_f64 2.00 (1.65);
apply_f64 and apply_n_f64: no element further than half an fp32 ulp from the longdouble result (0.00 beyond it), every form.

What the cases found:
  * test_stats_n[24-516-scales] (6.42 x), [129-516-scales] (6.66), [64-1729-scales] (5.78), [256-1729-scales] (5.50) and 29 more
    of the tile kernels' unmasked cases, test_stats_n_long[17-524356] (4.79) and [17-2097220] (5.20): cwctn_stats_tile_kernel
    summed a workgroup's 512 .. 2112 pixels in one fmaf chain per co-moment and one chain of row sums.  Every tile now has
    accumulators of its own.  test_stats_n[192-68-scales] then still sat at 4.02 through the mean: 16 dependent row-sum steps per
    tile; the row sums now go 4 pixels, 4 steps, 4 steps per tile (a CPU model of each order reproduced the device's figure).
  * test_stats_n[1-132-scales] (5.06 x; reg<4> otherwise up to 3.98, reg<16> 2.70).  N = 1, one workgroup, one pixel per thread:
    cwctn_stats_reg_kernel summed the workgroup in fp32 shuffle trees.  The first pixel, the shift, lies 1.93 standard deviations
    off the mean, so q - a^2 / n cancels 8.4-fold, and the tree's roundings (1.1 u in q) left 5.06 u in the variance (a CPU model
    of the order gave the device's bits).  The workgroup's sums now go through the shuffles in fp64 and are rounded to the fp32
    record once: the case sits at 0.12, the register kernels at the figures above."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cwct_any_ref as A                                               # noqa: E402
import cwct_ops_ref as O                                               # noqa: E402
from test_gpu_cwct_ops import (Guarded, at_offset, bits, dev, exact_constant_channel, ops,  # noqa: E402,F401
                               stop_at_a_device_error)

pytestmark = pytest.mark.gpu
B32 = O.FACTOR["stats"]


def same(a, b):
    return bits(a).tobytes() == bits(b).tobytes()


def exact_const(got, N):
    if N >= 3:
        exact_constant_channel(got, N)


def ident(v):
    return str(v)


# ================================================================================================= fp32 `_n`: statistics
_STATS = {}


def stats_refs(N, L, kind):
    key = (N, L, kind)
    if key not in _STATS:
        x = A.stats_input_n(N, L, kind)
        _STATS[key] = (x, O.stats64(x), O.stats32(x))
    return _STATS[key]


def run_stats(fn, x, off, N, mask=None, label=0):
    rec = Guarded((O.rec_len(N),), 0, dtype=torch.float64)
    xv = at_offset(x, off)
    fn(xv, mask=mask, label=label, out=rec.view)
    got = rec.check()
    fn(xv, mask=mask, label=label, out=rec.view)                      # a second call into the same buffers: the same bits
    assert same(rec.check(), got), "second call"
    return got


@pytest.mark.parametrize("N,L,kind", A.STATS_N_CASES, ids=ident)
def test_stats_n(ops, N, L, kind):
    x, want, r32 = stats_refs(N, L, kind)
    for off in A.STATS_OFFS:
        got = run_stats(ops.stats_n, x, off, N)
        r, (gc, gm, ec, em) = O.stats_ratio(got, r32, want, N, skip=A.skip_ch(N))
        print(f"stats_n N={N} L={L} off={off} {kind} [{A.stats_n_form(N)}]: e32 cov {ec / O.U:.3g} u mean {em / O.U:.3g} u, device cov "
              f"{gc / O.U:.3g} u mean {gm / O.U:.3g} u = {r:.2f} x max(e32, floor), bound {B32}")
        assert got[0] == L
        exact_const(got, N)
        assert r <= B32, (N, L, off, kind, r)


@pytest.mark.parametrize("N,L", A.LONG_N_CASES, ids=ident)
def test_stats_n_long(ops, N, L):
    x = A.long_input_n(N, L)
    want, r32 = O.stats64_chunked(x), O.stats32(x)
    got = ops.stats_n(dev(x)).cpu().numpy()
    r, (gc, gm, ec, em) = O.stats_ratio(got, r32, want, N, skip=A.skip_ch(N))
    print(f"stats_n N={N} L={L} [{A.stats_n_form(N)} long-{O.stats_groups(L)[2]}]: e32 cov {ec / O.U:.3g} u mean {em / O.U:.3g} u, "
          f"device cov {gc / O.U:.3g} u mean {gm / O.U:.3g} u = {r:.2f} x max(e32, floor), bound {B32}")
    assert got[0] == L
    exact_const(got, N)
    assert r <= B32, (N, L, r)


@pytest.mark.parametrize("N,L", A.MASK_N_CASES, ids=ident)
def test_stats_n_one_label(ops, N, L):
    x, mask = A.stats_input_n(N, L, "scales", seed=1), O.one_label_mask(L)
    dx = dev(x)
    for label in O.MASK_LABELS:
        sel = mask == label
        want, r32 = O.stats64(x, sel), O.stats32(x, mask, label)
        for moff in A.MASK_OFFS:
            got = ops.stats_n(dx, mask=at_offset(mask, moff, torch.uint8), label=label).cpu().numpy()
            r, (gc, gm, ec, em) = O.stats_ratio(got, r32, want, N, skip=A.skip_ch(N))
            print(f"stats_n N={N} L={L} label={label} ({int(sel.sum())} px) mask+{moff} [{A.stats_n_form(N)} label]: e32 cov "
                  f"{ec / O.U:.3g} u, device cov {gc / O.U:.3g} u mean {gm / O.U:.3g} u = {r:.2f} x, bound {B32}")
            assert got[0] == sel.sum()                                # the count is exact
            exact_const(got, N)
            assert r <= B32, (N, L, moff, label, r)


# ===================================================================================================== fp32 `_n`: factor
def run_factor(fn, content, styles, al, ac, N, min_tries=None, f64=False):
    aff = Guarded((N * N + N,), 0, dtype=torch.float64 if f64 else torch.float32)
    _, info = fn(dev(content), [dev(s) for s in styles], al, N, alpha_c=ac, eps=O.EPS, min_tries=min_tries, affine=aff.view)
    return aff.check(), info.cpu().tolist()


@pytest.mark.parametrize("N,k,ac,cond", A.FACTOR_N_CASES, ids=ident)
def test_factor_n(ops, N, k, ac, cond):
    content, styles, al = O.factor_input(N, k, cond)
    a32, info32 = O.factor32(content, styles, al, ac, N)
    ref = O.factor64(content, styles, al, ac, N, info32)
    e32 = O.factor_err(a32, ref, N)
    got, info = run_factor(ops.factor_n, content, styles, al, ac, N)
    r = O.ratio("factor", O.factor_err(got, ref, N), e32)
    print(f"factor_n N={N} styles={k} alpha_c={ac} cond={cond:g} [factor]: e32 {e32 / O.U:.3g} u, device = {r:.2f} x max(e32, floor), "
          f"bound {O.FACTOR['factor']}")
    assert info == info32                                             # retry counts (none here)
    assert r <= O.FACTOR["factor"], (N, k, ac, cond, r)
    again, info_a = run_factor(ops.factor_n, content, styles, al, ac, N)
    assert same(again, got) and info_a == info, "second call"
    # a prefactored style record gives the same affine bit for bit; prefactoring it again changes nothing; out may alias
    pre = Guarded((O.rec_len(N),), 0, dtype=torch.float64)
    _, pinfo = ops.prefactor_n(dev(styles[0]), N, O.EPS, out=pre.view)
    prec = pre.check()
    assert pinfo.cpu().tolist() == [0] and prec[0] == -(styles[0][0] + 1.0) and same(prec[1:1 + N], styles[0][1:1 + N])
    got2, info2 = run_factor(ops.factor_n, content, [prec] + styles[1:], al, ac, N)
    assert same(got2, got) and info2 == info, "prefactored"
    twice, tinfo = ops.prefactor_n(dev(prec), N, O.EPS)
    assert same(twice.cpu().numpy(), prec) and tinfo.cpu().tolist() == [0], "prefactored twice"
    alias = Guarded((O.rec_len(N),), 0, fill=styles[0], dtype=torch.float64)
    ops.prefactor_n(alias.view, N, O.EPS, out=alias.view)
    assert same(alias.check(), prec), "out aliases the record"


@pytest.mark.parametrize("kind", O.JITTER_KINDS)
@pytest.mark.parametrize("N", A.JITTER_N)
def test_factor_n_jitter(ops, N, kind):
    content = O.jitter_content(N, kind)
    _, styles, al = O.factor_input(N, 2, 10.0)
    a32, info32 = O.factor32(content, styles, al, 0.3, N)
    ref = O.factor64(content, styles, al, 0.3, N, info32)
    e32 = O.factor_err(a32, ref, N)
    got, info = run_factor(ops.factor_n, content, styles, al, 0.3, N)
    r = O.ratio("factor", O.factor_err(got, ref, N), e32)
    print(f"factor_n N={N} {kind} [factor jitter]: tries {info} (restatement {info32}), e32 {e32 / O.U:.3g} u, device = {r:.2f} x, "
          f"bound {O.FACTOR['factor']}")
    assert info == info32, "retry counts"
    assert r <= O.FACTOR["factor"], (N, kind, r)
    # the minimum-tries entry of info: the count itself changes nothing; more is kept, for the content and for a style
    same_a, info_s = run_factor(ops.factor_n, content, styles, al, 0.3, N, min_tries=[info[0], 0, 0, 0])
    assert info_s == info and same(same_a, got)
    mt = [info[0] + 2, 0, 1, 0]
    more, info_m = run_factor(ops.factor_n, content, styles, al, 0.3, N, min_tries=mt)
    a32m, info32m = O.factor32(content, styles, al, 0.3, N, min_tries=mt)
    assert info_m == info32m == mt
    refm = O.factor64(content, styles, al, 0.3, N, mt)
    rm = O.ratio("factor", O.factor_err(more, refm, N), O.factor_err(a32m, refm, N))
    print(f"factor_n N={N} {kind} min_tries {mt} [factor min_tries]: device = {rm:.2f} x")
    assert rm <= O.FACTOR["factor"]
    pre, pinfo = ops.prefactor_n(dev(content), N, O.EPS)              # the prefactor's retries are the factor's
    assert pinfo.cpu().tolist() == [info[0]]
    got2, info2 = run_factor(ops.factor_n, pre.cpu().numpy(), styles, al, 0.3, N)
    assert same(got2, got) and info2 == [0] + info[1:], "prefactored content"


@pytest.mark.parametrize("N", A.GIVE_UP_N)
def test_factor_n_gives_up(ops, N):
    """a NaN covariance fails every try at its first pivot: 4096 retries, the flag info[1]; the next call is untouched by it"""
    content, styles, al = O.factor_input(N, 1, 10.0)
    bad = content.copy()
    bad[1 + N:] = np.nan
    _, info = run_factor(ops.factor_n, bad, styles, al, 0.0, N)
    print(f"factor_n N={N} NaN covariance: info {info}")
    assert info == [4096, 1, 0]
    got, info = run_factor(ops.factor_n, content, styles, al, 0.0, N)
    a32, info32 = O.factor32(content, styles, al, 0.0, N)
    ref = O.factor64(content, styles, al, 0.0, N, info32)
    assert info == info32 == [0, 0, 0]
    assert O.ratio("factor", O.factor_err(got, ref, N), O.factor_err(a32, ref, N)) <= O.FACTOR["factor"]
    _, pinfo = ops.prefactor_n(dev(bad), N, O.EPS)
    assert pinfo.cpu().tolist() == [4096]


# ============================================================================================================== apply
APPLY_OFFS = ((0, 0), (1, 2), (2, 1), (4, 4))                          # (x, y) element offsets, each from (0, 1, 2, 4)


def apply_case(fn, x, aff, daff, mask, want, den, ratio_of, N, L, exact_t0):
    """every offset pair, out of place (sentinel-filled, guarded) and in place; returns the worst ratio"""
    on = np.ones(L, dtype=bool) if mask is None else mask == O.APPLY_LABEL
    dmask = None if mask is None else dev(mask)
    sent = np.full((N, L), O.SENTINEL_F32, dtype=np.float32)
    worst = 0.0
    for xo, yo in APPLY_OFFS:
        g = Guarded((N, L), yo, fill=sent)
        xv = at_offset(x, xo)
        fn(xv, daff, out=g.view, mask=dmask, label=O.APPLY_LABEL)
        got = g.check()
        worst = max(worst, ratio_of(got[:, on], on))
        assert same(got[:, ~on], sent[:, ~on]), "pixels of another label written"
        assert (got[:, O.ZERO_PIXEL] == exact_t0).all() and (N < 2 or (got[O.ZERO_ROW, on] == exact_t0[O.ZERO_ROW]).all())
        fn(xv, daff, out=g.view, mask=dmask, label=O.APPLY_LABEL)
        assert same(g.check(), got), "second call"
        gi = Guarded((N, L), xo, fill=x)                              # in place: the same bits, other labels keep x
        fn(gi.view, daff, out=gi.view, mask=dmask, label=O.APPLY_LABEL)
        goti = gi.check()
        assert same(goti[:, on], got[:, on]), ("in place", xo)
        assert same(goti[:, ~on], x[:, ~on]), ("in place, other labels", xo)
    return worst


@pytest.mark.parametrize("N,L,masked", A.APPLY_N_CASES, ids=ident)
def test_apply_n(ops, N, L, masked):
    x, aff = A.apply_input_n(N, L)
    mask = O.apply_mask(L) if masked else None
    want, den = O.apply64(x, aff, N)
    r32 = O.apply32(x, aff, N)

    def ratio_of(got, on):
        return O.ratio("apply", O.apply_err(got, want[:, on], den[:, on]), O.apply_err(r32[:, on], want[:, on], den[:, on]))
    r = apply_case(ops.apply_n, x, aff, dev(aff), mask, want, den, ratio_of, N, L, aff[N * N:])
    pg, lds, part = A.apply_n_form(N)
    print(f"apply_n N={N} L={L} masked={masked} [apply PG{pg}{' partial' if part else ''}]: e32 {O.apply_err(r32, want, den) / O.U:.3g} u, "
          f"device = {r:.2f} x max(e32, floor), bound {O.FACTOR['apply']}")
    assert r <= O.FACTOR["apply"], (N, L, masked, r)


# =================================================================================== agreement with the tuned kernels
@pytest.mark.parametrize("N", A.TUNED)
def test_n_calls_agree_with_the_tuned_calls(ops, N):
    """one input through both families; each is held to the bound"""
    for L, kind in ((516, "scales"), (1729, "scales"), (1729, "outlier")):
        x, want, r32 = stats_refs(N, L, kind)
        rn = O.stats_ratio(run_stats(ops.stats_n, x, 0, N), r32, want, N, skip=A.skip_ch(N))[0]
        rt = O.stats_ratio(run_stats(ops.stats, x, 0, N), r32, want, N, skip=A.skip_ch(N))[0]
        print(f"stats N={N} L={L} {kind} [agree stats]: _n = {rn:.2f} x, tuned = {rt:.2f} x, bound {B32}")
        assert rn <= B32 and rt <= B32, (N, L, kind, rn, rt)
    for k, ac, cond in ((1, 0.0, 1e4), (2, 0.3, 1e4)):
        content, styles, al = O.factor_input(N, k, cond)
        a32, info32 = O.factor32(content, styles, al, ac, N)
        ref = O.factor64(content, styles, al, ac, N, info32)
        e32 = O.factor_err(a32, ref, N)
        gn, info_n = run_factor(ops.factor_n, content, styles, al, ac, N)
        gt, info_t = run_factor(ops.factor, content, styles, al, ac, N)
        rn, rt = O.ratio("factor", O.factor_err(gn, ref, N), e32), O.ratio("factor", O.factor_err(gt, ref, N), e32)
        print(f"factor N={N} styles={k} alpha_c={ac} [agree factor]: _n = {rn:.2f} x, tuned = {rt:.2f} x, bound {O.FACTOR['factor']}")
        assert info_n == info_t == info32 and rn <= O.FACTOR["factor"] and rt <= O.FACTOR["factor"]
    for L in (65, 260):
        x, aff = O.apply_input(N, L)
        want, den = O.apply64(x, aff, N)
        e32 = O.apply_err(O.apply32(x, aff, N), want, den)
        gn = ops.apply_n(dev(x), dev(aff)).cpu().numpy()
        gt = ops.apply(dev(x), dev(aff), precision="fp32").cpu().numpy()
        rn, rt = O.ratio("apply", O.apply_err(gn, want, den), e32), O.ratio("apply", O.apply_err(gt, want, den), e32)
        print(f"apply N={N} L={L} [agree apply]: _n = {rn:.2f} x, tuned fp32 = {rt:.2f} x, bound {O.FACTOR['apply']}")
        assert rn <= O.FACTOR["apply"] and rt <= O.FACTOR["apply"]


# =============================================================================================================== fp64
def fam_fn(ops, fam, what):
    return getattr(ops, f"{what}_{fam}")


_STATS64 = {}


def stats64_refs(N, L, kind):
    """input, longdouble reference and float64 restatement of an unmasked case, shared by its offsets and by the two families"""
    key = (N, L, kind)
    if key not in _STATS64:
        x = A.stats_input_n(N, L, kind)
        _STATS64[key] = (x, A.stats_ld(x), A.stats_e64(x))
    return _STATS64[key]


@pytest.mark.parametrize("fam,N,L,kind", A.F64_STATS_CASES, ids=ident)
def test_stats_f64(ops, fam, N, L, kind):
    x, want, e64 = stats64_refs(N, L, kind)
    for off in A.STATS_OFFS:
        got = run_stats(fam_fn(ops, fam, "stats"), x, off, N)
        r, (gc, gm, ec, em) = A.stats64_ratio(got, e64, want, N, skip=A.skip_ch(N))
        print(f"stats_{fam} N={N} L={L} off={off} {kind} [{fam} stats, {A.chunks64(L)} chunks, grid.y {A.cov64n_blocks(N) if fam == 'n_f64' else 1}]: "
              f"e64 cov {ec / A.U64:.3g} u64 mean {em / A.U64:.3g} u64, device cov {gc / A.U64:.3g} u64 mean {gm / A.U64:.3g} u64 "
              f"= {r:.2f} x max(e64, 2^-53), bound {A.FACTOR64}")
        assert got[0] == L
        exact_const(got, N)
        assert r <= A.FACTOR64, (fam, N, L, off, kind, r)


@pytest.mark.parametrize("fam,N,L", A.F64_MASK_CASES, ids=ident)
def test_stats_f64_one_label(ops, fam, N, L):
    x, mask = A.stats_input_n(N, L, "scales", seed=1), O.one_label_mask(L)
    dx = dev(x)
    for label in O.MASK_LABELS:
        sel = mask == label
        key = (N, L, "label", label)
        if key not in _STATS64:
            _STATS64[key] = (A.stats_ld(x, sel), A.stats_e64(x, sel))
        want, e64 = _STATS64[key]
        for moff in A.MASK_OFFS:
            got = fam_fn(ops, fam, "stats")(dx, mask=at_offset(mask, moff, torch.uint8), label=label).cpu().numpy()
            r, (gc, gm, ec, em) = A.stats64_ratio(got, e64, want, N, skip=A.skip_ch(N))
            print(f"stats_{fam} N={N} L={L} label={label} ({int(sel.sum())} px) mask+{moff} [{fam} stats label]: e64 cov {ec / A.U64:.3g} u64, "
                  f"device cov {gc / A.U64:.3g} u64 mean {gm / A.U64:.3g} u64 = {r:.2f} x, bound {A.FACTOR64}")
            assert got[0] == sel.sum()
            exact_const(got, N)
            assert r <= A.FACTOR64, (fam, N, L, moff, label, r)


_FACTOR64 = {}


def factor64_refs(key, content, styles, al, ac, N, min_tries=None):
    if key not in _FACTOR64:
        a64, info = A.factor_e64(content, styles, al, ac, N, min_tries=min_tries)
        ref = A.factor_ld(content, styles, al, ac, N, info)
        _FACTOR64[key] = (ref, O.factor_err(a64, ref, N), info)
    return _FACTOR64[key]


@pytest.mark.parametrize("fam,N,k,ac,cond", A.F64_FACTOR_CASES, ids=ident)
def test_factor_f64(ops, fam, N, k, ac, cond):
    content, styles, al = O.factor_input(N, k, cond)
    ref, e64, info64 = factor64_refs((N, k, ac, cond), content, styles, al, ac, N)
    got, info = run_factor(fam_fn(ops, fam, "factor"), content, styles, al, ac, N, f64=True)
    r = A.ratio64(O.factor_err(got, ref, N), e64)
    print(f"factor_{fam} N={N} styles={k} alpha_c={ac} cond={cond:g} [{fam} factor]: e64 {e64 / A.U64:.3g} u64, device = {r:.2f} x "
          f"max(e64, 2^-53), bound {A.FACTOR64}")
    assert info == info64
    assert r <= A.FACTOR64, (fam, N, k, ac, cond, r)
    again, info_a = run_factor(fam_fn(ops, fam, "factor"), content, styles, al, ac, N, f64=True)
    assert same(again, got) and info_a == info, "second call"


@pytest.mark.parametrize("kind", O.JITTER_KINDS)
@pytest.mark.parametrize("fam,N", A.F64_JITTER_CASES, ids=ident)
def test_factor_f64_jitter(ops, fam, N, kind):
    content = O.jitter_content(N, kind)
    _, styles, al = O.factor_input(N, 2, 10.0)
    ref, e64, info64 = factor64_refs((N, kind), content, styles, al, 0.3, N)
    fn = fam_fn(ops, fam, "factor")
    got, info = run_factor(fn, content, styles, al, 0.3, N, f64=True)
    r = A.ratio64(O.factor_err(got, ref, N), e64)
    print(f"factor_{fam} N={N} {kind} [{fam} factor jitter]: tries {info} (restatement {info64}), e64 {e64 / A.U64:.3g} u64, device = {r:.2f} x, "
          f"bound {A.FACTOR64}")
    assert info == info64, "retry counts"
    assert r <= A.FACTOR64, (fam, N, kind, r)
    same_a, info_s = run_factor(fn, content, styles, al, 0.3, N, min_tries=[info[0], 0, 0, 0], f64=True)
    assert info_s == info and same(same_a, got)
    mt = [info[0] + 2, 0, 1, 0]
    refm, e64m, info64m = factor64_refs((N, kind, "more"), content, styles, al, 0.3, N, min_tries=mt)
    more, info_m = run_factor(fn, content, styles, al, 0.3, N, min_tries=mt, f64=True)
    rm = A.ratio64(O.factor_err(more, refm, N), e64m)
    print(f"factor_{fam} N={N} {kind} min_tries {mt} [{fam} factor min_tries]: device = {rm:.2f} x")
    assert info_m == info64m == mt and rm <= A.FACTOR64


_APPLY64 = {}


@pytest.mark.parametrize("fam,N,L,masked", A.F64_APPLY_CASES, ids=ident)
def test_apply_f64(ops, fam, N, L, masked):
    x, aff = A.apply_input_n(N, L, f64=True)
    if (N, L) not in _APPLY64:
        want, den = A.apply_ld(x, aff, N)
        _APPLY64[(N, L)] = (want, den, A.apply_e64(x, aff, N))
    want, den, y64 = _APPLY64[(N, L)]
    mask = O.apply_mask(L) if masked else None

    def ratio_of(got, on):
        return A.apply64_ratio(got, A.apply64_e64(y64[:, on], want[:, on], den[:, on]), want[:, on], den[:, on])
    r = apply_case(fam_fn(ops, fam, "apply"), x, aff, dev(aff), mask, want, den, ratio_of, N, L, aff[N * N:].astype(np.float32))
    e64 = A.apply64_e64(y64, want, den)
    form = f"PG{A.apply_n_form(N)[0]}{' partial' if A.apply_n_form(N)[2] else ''}" if fam == "n_f64" else "pixel per thread"
    print(f"apply_{fam} N={N} L={L} masked={masked} [{fam} apply {form}]: e64 {e64 / A.U64:.3g} u64, device beyond half an fp32 ulp "
          f"= {r:.2f} x max(e64, 2^-53), bound {A.FACTOR64}")
    assert r <= A.FACTOR64, (fam, N, L, masked, r)
