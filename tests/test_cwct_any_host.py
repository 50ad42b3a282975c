"""The per-kernel tests of csrc/cwct_any.hip and csrc/cwct64.hip, host side (tests/cwct_any_ref.py; the GPU side is
tests/test_gpu_cwct_ops_any.py).

The case tables reach every launch form of the two files (every statistics kernel and channel-block count, every PG of the
apply, both grid shapes of the fp64 covariance, one to three fp64 chunks, all four group regimes); np.longdouble has a 64-bit
mantissa here (a machine without it fails, it does not pass vacuously); the restatements sit at <= 1 x max(e, floor) and the
`_n` restatements without a switch are O's own bits; every mutant exceeds 1.25 x its factor at one case of the tables; the
wrappers refuse bad arguments without a GPU and call only what include/vstnet.h declares.  Every test prints its figures (-s)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cwct_any_ref as A                                               # noqa: E402
import cwct_ops_ref as O                                               # noqa: E402

TEETH = 1.25
NAMES = ["vst_cwct_stats_n", "vst_cwct_factor_n", "vst_cwct_prefactor_n", "vst_cwct_apply_n", "vst_cwct_stats_f64",
         "vst_cwct_factor_f64", "vst_cwct_apply_f64", "vst_cwct_stats_n_f64", "vst_cwct_factor_n_f64", "vst_cwct_apply_n_f64"]
SIZES = ["vst_cwct_stats_n_workspace_bytes", "vst_cwct_factor_n_workspace_bytes", "vst_cwct_stats_f64_workspace_bytes",
         "vst_cwct_factor_f64_workspace_bytes", "vst_cwct_stats_n_f64_workspace_bytes", "vst_cwct_factor_n_f64_workspace_bytes"]


def built_library():
    from vstnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def note(worst, m, v, case):
    if v > worst[m][0]:
        worst[m] = (v, case)


def check_teeth(what, worst, factor):
    for m, (v, case) in worst.items():
        print(f"{what} mutant '{m}': {v:.3g} x at {case} (needs > {TEETH * factor})")
        assert v > TEETH * factor, (m, v, case)


def test_longdouble_has_a_64_bit_mantissa():
    eps = np.finfo(np.longdouble).eps
    print(f"np.longdouble: eps = 2^{np.log2(float(eps)):.0f}")
    assert eps <= 2.0 ** -63, "the fp64 references need extended precision"


# ------------------------------------------------------------------------------------------------------------- forms
def test_case_tables_reach_every_launch_form():
    for form, widths in A.STATS_N_WIDTHS.items():
        assert {A.stats_n_form(N) for N in widths} == {form}, form
    assert set(A.STATS_N_WIDTHS) == {A.stats_n_form(N) for N in range(1, 257)}             # no form is left out
    nb = {(N + A.stats_n_block(N) - 1) // A.stats_n_block(N) for N in A.STATS_N if A.stats_n_block(N)}
    assert nb == {1, 2, 3, 4}
    for a, b in ((4, 5), (8, 9), (16, 17), (32, 33), (64, 65), (128, 129), (192, 193)):     # both sides of every threshold
        assert a in A.STATS_N and b in A.STATS_N and A.stats_n_form(a) != A.stats_n_form(b)
    regimes = {O.stats_groups(L)[2] for L in O.STATS_L} | {O.stats_groups(L)[2] for _, L in A.LONG_N_CASES}
    assert regimes == {"512", "1024", "2048", "capped"}, regimes
    assert {O.stats_groups(L)[2] for N, L in A.LONG_N_CASES if N == 17} == {"1024", "2048", "capped"}
    assert O.stats_groups(A.LONG_N_CASES[0][1])[1] == 2112                                   # the capped regime's 33 tiles

    pg = {}
    for N in A.APPLY_N:
        pg.setdefault(A.apply_n_form(N)[0], []).append(N)
    print("apply PG:", pg)
    assert set(pg) == {4, 2, 1}
    assert [A.apply_n_form(N)[0] for N in (32, 33, 64, 65)] == [4, 2, 2, 1]
    assert A.apply_n_form(240)[1] < 65536 == A.apply_n_form(241)[1] == A.apply_n_form(256)[1]
    assert all(any(A.apply_n_form(N)[2] == part for N in ns) for ns in pg.values() for part in (False, True))
    for fam in ("f64", "n_f64"):
        assert set(A.F64_N[fam]) <= set(range(1, 257))
    assert {A.cov64n_blocks(N) for N in A.F64_N["n_f64"]} >= {1, 2, 64} and A.cov64n_blocks(32) == 1 < A.cov64n_blocks(33)
    assert {A.chunks64(L) for L in A.F64_STATS_L} == {1, 2, 3}
    assert (A.chunks64(2048), A.chunks64(2049)) == (1, 2)
    assert {N for N, *_ in A.FACTOR_N_CASES} == set(A.FACTOR_N) and not any(N == 256 and k == 8 for N, k, _, _ in A.FACTOR_N_CASES)


# ------------------------------------------------------------------------------------------------------ fp32, `_n`
def test_stats_n_restatement_and_mutants():
    worst = {m: (0.0, None) for m in A.MUTANTS["stats_n"]}
    for N in (1, 3, 12, 24, 100, 160):
        for L, kind in ((68, "scales"), (516, "scales"), (1729, "scales"), (1729, "outlier")):
            x = A.stats_input_n(N, L, kind)
            want, r32 = O.stats64(x), A.stats32_n(x)
            assert r32.tobytes() == O.stats32(x).tobytes()                     # without a switch: O's restatement
            r, (gc, gm, ec, em) = O.stats_ratio(r32, r32, want, N, skip=A.skip_ch(N))
            print(f"stats_n N={N} L={L} {kind} [{A.stats_n_form(N)}]: e32 cov {ec / O.U:.3g} u, mean {em / O.U:.3g} u, "
                  f"restatement {r:.2f} x")
            assert r <= 1.0 and r32[0] == L
            for m in A.MUTANTS["stats_n"][:3]:
                got = A.stats32_n(x, mut=(m,))
                note(worst, m, O.stats_ratio(got, r32, want, N, skip=A.skip_ch(N))[0], (N, L, kind))
    for N in (3, 24, 100):
        for L in O.MASK_L:
            x, mask = A.stats_input_n(N, L, "scales", seed=1), O.one_label_mask(L)
            for lab in O.MASK_LABELS:
                want, r32 = O.stats64(x, mask == lab), A.stats32_n(x, mask, lab)
                assert r32.tobytes() == O.stats32(x, mask, lab).tobytes() and r32[0] == (mask == lab).sum()
                for m in A.MUTANTS["stats_n"]:
                    got = A.stats32_n(x, mask, lab, mut=(m,))
                    note(worst, m, O.stats_ratio(got, r32, want, N, skip=A.skip_ch(N))[0], (N, L, "label", lab))
    check_teeth("stats_n", worst, O.FACTOR["stats"])


def test_narrow_inputs_are_what_they_claim():
    for N in (1, 2):
        x = A.stats_input_n(N, 516)
        assert x.shape == (N, 516) and (x.std(1) > 0).all()                   # no constant channel below 3 channels
        assert N == 1 or abs(np.corrcoef(x)[0, 1]) < 0.5                      # ... and no collinear one
    x = A.stats_input_n(3, 516)
    assert (x[O.CONST_CH] == O.CONST_VAL).all() and A.skip_ch(3) == (O.CONST_CH,) and A.skip_ch(1) == ()
    x = A.long_input_n(5, 4096)
    assert x.shape == (5, 4096) and (x[O.CONST_CH] == O.CONST_VAL).all()
    assert A.long_input_n(32, 70000).tobytes() == O.long_input(70000).tobytes()
    x, aff = A.apply_input_n(1, 5)
    assert x.shape == (1, 5) and aff.shape == (2,) and aff.dtype == np.float32 and x[0, O.ZERO_PIXEL] == 0
    x, aff = A.apply_input_n(17, 5, f64=True)
    assert aff.dtype == np.float64 and (aff != aff.astype(np.float32)).any() and not aff[17:34].any()


def test_apply_n_restatement_and_mutants():
    worst = {m: (0.0, None) for m in A.MUTANTS["apply_n"]}
    for N in A.APPLY_N:
        for L in (3, 65, 260):
            x, aff = A.apply_input_n(N, L)
            want, den = O.apply64(x, aff, N)
            r32 = A.apply32_n(x, aff, N)
            assert r32.tobytes() == O.apply32(x, aff, N).tobytes()
            e32 = O.apply_err(r32, want, den)
            print(f"apply_n N={N} L={L} [PG {A.apply_n_form(N)[0]}]: e32 {e32 / O.U:.3g} u")
            assert (r32[:, O.ZERO_PIXEL] == aff[N * N:]).all()
            for m in worst:
                note(worst, m, O.ratio("apply", O.apply_err(A.apply32_n(x, aff, N, mut=(m,)), want, den), e32), (N, L))
    check_teeth("apply_n", worst, O.FACTOR["apply"])


# -------------------------------------------------------------------------------------------------------------- fp64
def test_stats_f64_restatement_and_mutants():
    worst = {m: (0.0, None) for m in A.MUTANTS["stats_f64"]}
    for N, L, kind in ((1, 516, "scales"), (3, 2049, "scales"), (24, 68, "scales"), (24, 4100, "scales"), (33, 1729, "outlier"),
                       (64, 2048, "scales")):
        x = A.stats_input_n(N, L, kind)
        want, e64 = A.stats_ld(x), A.stats_e64(x)
        r, (gc, gm, ec, em) = A.stats64_ratio(e64, e64, want, N, skip=A.skip_ch(N))
        print(f"stats_f64 N={N} L={L} {kind}: e64 cov {ec / A.U64:.3g} u64, mean {em / A.U64:.3g} u64, restatement {r:.2f} x")
        assert r <= 1.0 and e64[0] == L and ec < 1e-10 and em < 1e-10
        d32 = O.stats_err(O.stats64(x), want, N, skip=A.skip_ch(N))            # numpy's fp64 two-pass sits at the same level
        assert d32[0] < 1e-10
        for m in worst:
            note(worst, m, A.stats64_ratio(A.stats_e64(x, mut=(m,)), e64, want, N, skip=A.skip_ch(N))[0], (N, L, kind))
    x, mask = A.stats_input_n(24, 4100, "scales", seed=1), O.one_label_mask(4100)
    for lab in O.MASK_LABELS:
        sel = mask == lab
        want, e64 = A.stats_ld(x, sel), A.stats_e64(x, sel)
        assert e64[0] == sel.sum() and A.stats64_ratio(e64, e64, want, 24, skip=A.skip_ch(24))[0] <= 1.0
    check_teeth("stats_f64", worst, A.FACTOR64)


def test_factor_f64_restatement_and_mutants():
    worst = {m: (0.0, None) for m in A.MUTANTS["factor_f64"]}
    for N, k, ac, cond in ((1, 1, 0.0, 1e1), (3, 2, 0.3, 1e4), (24, 8, 0.3, 1e4), (100, 2, 0.0, 1e4)):
        content, styles, al = O.factor_input(N, k, cond)
        a64, info = A.factor_e64(content, styles, al, ac, N)
        ref = A.factor_ld(content, styles, al, ac, N, info)
        e64 = O.factor_err(a64, ref, N)
        T64, t64 = O.factor64(content, styles, al, ac, N, info)[:2]
        d = O.factor_err(np.concatenate([np.tril(T64).reshape(-1), t64]), ref, N)
        print(f"factor_f64 N={N} styles={k} alpha_c={ac} cond={cond:g}: e64 {e64 / A.U64:.3g} u64 (LAPACK in fp64: {d / A.U64:.3g})")
        assert info == [0] * (2 + k) and e64 < 1e-9 and d < 1e-9
    for N in (12, 24, 100):
        for kind in O.JITTER_KINDS:
            content = O.jitter_content(N, kind)
            _, styles, al = O.factor_input(N, 2, 10.0)
            a64, info = A.factor_e64(content, styles, al, 0.3, N)
            assert info[0] == {"rank_deficient": 2, "constant_channel": 1, "indefinite": 3}[kind] and info[1:] == [0, 0, 0]
            ref = A.factor_ld(content, styles, al, 0.3, N, info)
            e64 = O.factor_err(a64, ref, N)
            got, info_m = A.factor_e64(content, styles, al, 0.3, N, mut=("jitter_not_cumulative",))
            note(worst, "jitter_not_cumulative", A.ratio64(O.factor_err(got, ref, N), e64), (N, kind, info_m))
            print(f"factor_f64 N={N} {kind}: tries {info}, e64 {e64 / A.U64:.3g} u64")
            assert A.factor_e64(content, styles, al, 0.3, N, min_tries=[info[0] + 2, 0, 1, 0])[1] == [info[0] + 2, 0, 1, 0]
    # the jitter steps are fp32 values (some t eps need more than 24 bits), and the longdouble reference follows the rounding
    st = A.jitter_steps(16, O.EPS)
    assert all(s == float(np.float32(s)) for s in st) and any(s != (t + 1) * float(np.float32(O.EPS)) for t, s in enumerate(st))
    check_teeth("factor_f64", worst, A.FACTOR64)


def test_apply_f64_restatement_and_mutants():
    worst = {m: (0.0, None) for m in A.MUTANTS["apply_f64"]}
    for N in (1, 3, 24, 32, 33, 100):
        for L in (3, 65, 260):
            x, aff = A.apply_input_n(N, L, f64=True)
            want, den = A.apply_ld(x, aff, N)
            y64 = A.apply_e64(x, aff, N)
            e64 = A.apply64_e64(y64, want, den)
            r = A.apply64_ratio(y64.astype(np.float32), e64, want, den)
            print(f"apply_f64 N={N} L={L}: e64 {e64 / A.U64:.3g} u64, restatement rounded to fp32 {r:.2f} x")
            assert r <= 1.0 and e64 < 64 * A.U64
            for m in worst:
                got = A.apply_e64(x, aff, N, mut=(m,)).astype(np.float32)
                note(worst, m, A.apply64_ratio(got, e64, want, den), (N, L))
    # half an ulp of float32, at the binade's lower edge and just below it
    assert A.half_ulp32(np.array([1.0, 1.9999, 0.99999, 0.0]))[:3].tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -25]
    check_teeth("apply_f64", worst, A.FACTOR64)


# ---------------------------------------------------------------------------------------------------------- wrappers
def test_wrappers_call_what_the_header_declares():
    from vstnet_amd import _lib, cwct, cwct_ops_any
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    src = open(os.path.join(REPO, "vstnet_amd", "cwct_ops_any.py")).read()
    used = set(re.findall(r"\"(vst_[a-z0-9_]+)\"", src)) | set(re.findall(r"\.(vst_[a-z0-9_]+)\(", src))
    assert used == set(NAMES) | {"vst_cwct_factor_n_workspace_bytes"}, used ^ set(NAMES)
    L = built_library()
    for name in NAMES + SIZES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr) and name in _lib.EXPORTS, name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in NAMES:
        fn = name[len("vst_cwct_"):]
        assert getattr(cwct.ops, fn) is getattr(cwct_ops_any, fn), fn


def test_wrapper_refusals_need_no_gpu():
    from vstnet_amd import cwct_ops as ops
    x = torch.zeros(24, 68)
    rec = lambda n, dt=torch.float64: torch.zeros(1 + n + n * n, dtype=dt)      # noqa: E731
    for stats in (ops.stats_n, ops.stats_n_f64):
        for bad, msg in ((x.double(), "float32"), (x.t(), "contiguous"), (x[0], r"\[N, L\]"), (x, "CUDA"), (torch.zeros(257, 4), "1..256"),
                         (torch.zeros(0, 4), "1..256")):
            with pytest.raises(ValueError, match=msg):
                stats(bad)
        with pytest.raises(ValueError, match="shape"):
            stats(x, mask=torch.zeros(67, dtype=torch.uint8))
        with pytest.raises(ValueError, match="shape"):
            stats(x, out=rec(23))
    with pytest.raises(ValueError, match="one of"):
        ops.stats_f64(x)
    with pytest.raises(ValueError, match="CUDA"):
        ops.stats_f64(torch.zeros(32, 68))
    assert x.reshape(-1)[1:1 + 24 * 16].view(24, 16).is_contiguous()           # a view at an element offset is what they accept
    for factor, n in ((ops.factor_n, 24), (ops.factor_n_f64, 24), (ops.factor_f64, 32)):
        with pytest.raises(ValueError, match="float64"):
            factor(rec(n, torch.float32), [rec(n)], [1.0], n)
        with pytest.raises(ValueError, match="styles"):
            factor(rec(n), [], [], n)
        with pytest.raises(ValueError, match="styles"):
            factor(rec(n), [rec(n)] * 9, [1.0] * 9, n)
        with pytest.raises(ValueError, match="shape"):
            factor(rec(n), [rec(n + 1)], [1.0], n)
        with pytest.raises(ValueError, match="CUDA"):
            factor(rec(n), [rec(n)], [1.0], n)
    with pytest.raises(ValueError, match="float64"):                           # the fp64 affine is double [N*N + N]
        ops.factor_n_f64(rec(24), [rec(24)], [1.0], 24, affine=torch.zeros(24 * 24 + 24))
    with pytest.raises(ValueError, match="float32"):
        ops.factor_n(rec(24), [rec(24)], [1.0], 24, affine=torch.zeros(24 * 24 + 24, dtype=torch.float64))
    with pytest.raises(ValueError, match="one of"):
        ops.factor_f64(rec(24), [rec(24)], [1.0], 24)
    with pytest.raises(ValueError, match="1..256"):
        ops.factor_n(rec(257), [rec(257)], [1.0], 257)
    with pytest.raises(ValueError, match="shape"):
        ops.prefactor_n(rec(24), 23)
    with pytest.raises(ValueError, match="CUDA"):
        ops.prefactor_n(rec(24), 24)
    with pytest.raises(ValueError, match="float32"):
        ops.apply_n(x, torch.zeros(24 * 24 + 24, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        ops.apply_n_f64(x, torch.zeros(24 * 24 + 24))
    with pytest.raises(ValueError, match="shape"):
        ops.apply_n_f64(x, torch.zeros(24 * 24, dtype=torch.float64))
    with pytest.raises(ValueError, match="one of"):
        ops.apply_f64(x, torch.zeros(24 * 24 + 24, dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        ops.apply_n(x, torch.zeros(24 * 24 + 24), out=torch.zeros(24, 67))
    with pytest.raises(ValueError, match="CUDA"):
        ops.apply_n(x, torch.zeros(24 * 24 + 24))
    # the library's own refusals come before any launch
    import ctypes as C
    L = built_library()
    ok, null = C.c_void_p(4096), C.c_void_p(0)
    need = L.vst_cwct_stats_n_workspace_bytes(24, 68)
    assert need == O.stats_groups(68)[0] * (24 * 24 + 2 * 24 + 4) * 4 and L.vst_cwct_stats_n_workspace_bytes(257, 68) == 0
    assert L.vst_cwct_stats_n(ok, 257, 68, null, 0, ok, ok, 1 << 30, null) == -2 and L.vst_cwct_stats_n(ok, 24, 0, null, 0, ok, ok, need, null) == -1
    assert L.vst_cwct_stats_n(ok, 24, 68, null, 0, ok, ok, need - 1, null) == -4
    assert L.vst_cwct_stats_n_f64(ok, 24, 68, null, 0, ok, ok, L.vst_cwct_stats_n_f64_workspace_bytes(24, 68) - 1, null) == -4
    assert L.vst_cwct_stats_f64(ok, 24, 68, null, 0, ok, ok, null) == -2
    assert L.vst_cwct_apply_f64(ok, ok, 24, 68, ok, null, 0, null) == -2 and L.vst_cwct_apply_n(ok, ok, 0, 68, ok, null, 0, null) == -2
    assert L.vst_cwct_prefactor_n(ok, 24, 2e-5, ok, ok, ok, L.vst_cwct_factor_n_workspace_bytes(24) - 1, null) == -4
