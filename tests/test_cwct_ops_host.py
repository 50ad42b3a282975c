"""The per-kernel cWCT tests, host side (tests/cwct_ops_ref.py; the GPU side is tests/test_gpu_cwct_ops.py).

The case tables reach every launch form of csrc/cwct.hip (the launch conditions are restated in cwct_ops_ref.py); the fp32
restatements sit at or under FACTOR / 2 of max(e32, floor) at every case (e32 IS the restatement's error, so that is the floor
rule at work) and every mutant of them exceeds 1.25 x FACTOR at one case at least; the special inputs are what they claim; the
fp64 references compose into oracle/cpu_ref.transfer and transfer_seg; the wrappers refuse bad arguments without a GPU and call
only what include/vstnet.h declares.  Every test prints its figures (-s)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cwct_ops_ref as O                                               # noqa: E402

TEETH = 1.25
NAMES = ["vst_cwct_stats_workspace_bytes", "vst_cwct_stats", "vst_cwct_factor", "vst_cwct_prefactor", "vst_cwct_apply_prec",
         "vst_label_plan", "vst_cwct_labels_workspace_bytes", "vst_cwct_stats_labels", "vst_cwct_factor_labels",
         "vst_cwct_factor_labels_keyed", "vst_cwct_factor_labels_mix", "vst_cwct_apply_labels", "vst_z_to_code", "vst_mask_to_code",
         "vst_cwct_stats_code_workspace_bytes", "vst_cwct_stats_code", "vst_cwct_stats_code_rect", "vst_cwct_apply_code",
         "vst_cwct_stats_labels_code_workspace_bytes", "vst_cwct_stats_labels_code", "vst_cwct_stats_labels_code_rect",
         "vst_cwct_apply_labels_code"]


def built_library():
    from vstnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def check_teeth(op, worst, mutants):
    for m in mutants:
        print(f"{op} mutant '{m}': {worst[m][0]:.3g} x at {worst[m][1]} (needs > {TEETH * O.FACTOR[op]})")
        assert worst[m][0] > TEETH * O.FACTOR[op], (m, worst[m])


def note(worst, m, v, case):
    if v > worst[m][0]:
        worst[m] = (v, case)


# ------------------------------------------------------------------------------------------------------------- forms
def test_case_tables_reach_every_launch_form():
    stats = {(O.stats_form(N, L, off), min(N, 32)) for N, L, off, _ in O.STATS_CASES}
    stats |= {(O.stats_form(N, L, 0, moff), min(N, 32)) for N, L, moff, _ in O.MASK_CASES}
    assert stats >= {("fma16", 16), ("mfma_vec", 32), ("mfma_scalar", 32)}
    for N in (32, 64, 128):                       # VEC and not, each decided by L % 4, x % 16 and mask % 4 in turn
        assert {O.stats_form(N, L, off) for n, L, off, _ in O.STATS_CASES if n == N} == {"mfma_vec", "mfma_scalar"}
        assert O.stats_form(N, 68, 1) == "mfma_scalar" and O.stats_form(N, 65, 0) == "mfma_scalar"
        assert {O.stats_form(N, L, 0, moff) for n, L, moff, _ in O.MASK_CASES if n == N and L % 4 == 0} == {"mfma_vec", "mfma_scalar"}
    regimes = {O.stats_groups(L)[2] for L in O.STATS_L + O.STATS_LONG}
    assert regimes == {"512", "1024", "2048", "capped"}, regimes
    assert {O.stats_groups(L)[0] for L in O.STATS_L} >= {1, 2, 4}          # one workgroup, a second one of 4 pixels, several
    assert O.stats_groups(516) == (2, 512, "512") and O.stats_groups(1729)[0] == 4

    forms = {}
    for N, L, prec, masked in O.APPLY_CASES:
        for off in O.APPLY_OFFS:
            forms.setdefault(O.apply_form(N, L, off, off, masked, prec), []).append((N, L, prec, masked, off))
    print("apply forms:", {k: len(v) for k, v in forms.items()})
    assert set(forms) == {"split", "mfma4", "mfma2", "mfma1", "fma_vec", "fma_scalar"}
    assert {c[0] for c in forms["split"]} == {64, 128}
    assert any(c[:2] == (128, 4096 + 64) for c in forms["split"])           # several split iterations per wave, grid stride
    assert {c[0] for c in forms["fma_vec"]} == {16}                         # (N >= 32 with vector-aligned rows takes the MFMA form)
    assert {c[0] for c in forms["fma_scalar"]} == {16, 32, 64}

    lab = {}
    for N, L, prec, n, ms, kind in O.APPLY_LABELS_CASES:
        f, passes = O.apply_labels_form(N, L, 0, 0, 0, prec, ms)
        lab.setdefault((N, f), set()).add(passes)
    for N, L, prec, n, ms, kind in O.APPLY_LABELS_CASES:                    # the same cases with x and y one element in
        lab.setdefault((N, O.apply_labels_form(N, L, 1, 1, 0, prec, ms)[0]), set())
    print("apply_labels forms:", lab)
    assert set(lab) == {(32, "split"), (32, "v4"), (32, "v1"), (64, "split"), (64, "v2"), (64, "v1"), (128, "split"), (128, "v2"),
                        (128, "v1")}
    assert lab[(32, "split")] >= {1, 2, 4} and lab[(64, "v2")] >= {1, 2, 8} and lab[(128, "split")] >= {1, 2, 32}
    passes = {N: {O.stats_labels_passes(N, ms) for n, L, c, ms, k in O.PLAN_CASES if n == N} for N in (32, 64, 128)}
    assert passes[32] >= {1, 2, 4} and passes[64] >= {1, 2, 8} and passes[128] >= {1, 2, 32}, passes   # the 4th pass of 32 slots

    code = {O.stats_code_form(H, W, sp, r) for sp, H, W, r in O.CODE_CASES}
    assert code == {"pm", "pm_rect", "pm128", "pm128_rect"}
    assert {(sp, O.code_groups(H, W, sp)[0] > O.code_groups(H, W, sp)[1]) for sp, H, W, _ in O.CODE_CASES} >= \
        {(1, False), (1, True), (2, False), (2, True)}                       # one workgroup and several, both widths


# -------------------------------------------------------------------------------------------------------- statistics
def test_stats_restatement_and_mutants():
    worst = {m: (0.0, None) for m in O.MUTANTS["stats"]}
    for N, L, off, kind in O.STATS_CASES:
        if off:
            continue                               # the offset changes the form, not the restatement
        x = O.stats_input(N, L, kind)
        want = O.stats64(x)
        r32 = O.stats32(x)
        r, (gc, gm, ec, em) = O.stats_ratio(r32, r32, want, N, skip=(O.CONST_CH,))
        print(f"stats N={N} L={L} {kind}: e32 cov {ec / O.U:.3g} u, mean {em / O.U:.3g} u, restatement {r:.2f} x")
        assert r <= O.FACTOR["stats"] / 2
        _, m32, c32 = O.unpack(r32, N)
        assert r32[0] == L and m32[O.CONST_CH] == O.CONST_VAL and not c32[O.CONST_CH].any() and not c32[:, O.CONST_CH].any()
        if N in (16, 32) and L >= 63:
            for m in O.MUTANTS["stats"][:4]:
                note(worst, m, O.stats_ratio(O.stats32(x, mut=(m,)), r32, want, N, skip=(O.CONST_CH,))[0], (N, L, kind))
    for N, L, moff, lab in O.MASK_CASES:
        if moff or N not in (16, 32):
            continue
        x, mask = O.stats_input(N, L, "scales", seed=1), O.one_label_mask(L)
        want, r32 = O.stats64(x, mask == lab), O.stats32(x, mask, lab)
        assert r32[0] == want[0] == (mask == lab).sum()
        for m in O.MUTANTS["stats"]:
            got = O.stats32(x, mask, lab, mut=(m,), vec=O.stats_form(N, L, 0, 0) == "mfma_vec")
            note(worst, m, O.stats_ratio(got, r32, want, N, skip=(O.CONST_CH,))[0], (N, L, "label", lab))
    check_teeth("stats", worst, O.MUTANTS["stats"])


def test_stats_long_cases():
    """the 1024- and 2048-pixel groups and the capped branch: the restatement in chunks keeps a case at a few seconds"""
    L = O.STATS_LONG[0]
    x = O.long_input(L)
    want, r32 = O.stats64_chunked(x), O.stats32(x)
    r, figs = O.stats_ratio(r32, r32, want, 32, skip=(O.CONST_CH,))
    print(f"stats N=32 L={L}: e32 cov {figs[2] / O.U:.3g} u, mean {figs[3] / O.U:.3g} u")
    assert r <= O.FACTOR["stats"] / 2 and r32[0] == L
    got = O.stats32(x, mut=("record_dropped",))
    assert O.stats_ratio(got, r32, want, 32, skip=(O.CONST_CH,))[0] > TEETH * O.FACTOR["stats"]
    small = x[:, :5000]
    assert np.allclose(O.stats64_chunked(small, chunk=777), O.stats64(small), rtol=1e-12, atol=1e-14)


def test_stats_labels_restatement_and_mutants():
    muts = O.MUTANTS["stats"][1:4] + O.MUTANTS["stats_labels"]          # (the combine is shared with the one-label form)
    worst = {m: (0.0, None) for m in muts}
    for N, L, n, ms, kind in O.PLAN_CASES:
        x = O.plan_input(N, L)
        cm, sm = O.plan_mask(L, n, kind, N)
        lut, labels, over = O.plan_ref(cm, sm)
        assert len(labels) == n and not over and labels == O.plan_labels(n), (N, L, n, kind, labels)
        if N == 128 and n == 32 and kind != "runs":
            continue                               # 32 passes of the same arithmetic: one kind is enough on the host
        want, r32 = O.stats_labels64(x, cm, lut, n), O.stats_labels32(x, cm, lut, n, ms)
        assert (r32[n:] == O.SENTINEL_F64).all() and (r32[:n, 0] == want[:n, 0]).all()
        e = max(O.stats_err(r32[s], want[s], N, skip=(O.CONST_CH,))[0] for s in range(n))
        print(f"stats_labels N={N} L={L} slots={n} max_slots={ms} {kind}: e32 cov {e / O.U:.3g} u")
        if N == 32 or (N == 64 and L == 1092):
            for m in muts:
                got = O.stats_labels32(x, cm, lut, n, ms, mut=(m,))
                v = max(O.stats_ratio(got[s], r32[s], want[s], N, skip=(O.CONST_CH,))[0] if got[s, 0] != O.SENTINEL_F64 else np.inf
                        for s in range(n))
                note(worst, m, v, (N, L, n, ms, kind))
    check_teeth("stats", worst, muts)


def test_plan_masks_are_what_they_claim():
    for N in (32, 64, 128):
        k = O.KRES[N]
        for L in O.PLAN_L:
            _, per, _ = O.stats_groups(L)
            for n in (max(k, 2), k + 1):
                cm, sm = O.plan_mask(L, n, "runs", N)
                sl = O.plan_ref(cm, sm)[0][cm]
                rem = {(s, int((sl[a:min(a + 64, b)] == s).sum()) % 4) for w in range(0, L, per) for b in [min(w + per, L)]
                       for a in range(w, b, 64) for s in range(n)}
                assert all((s, 1) in rem for s in range(n)), (N, L, n)   # every slot meets a tile where it needs all 3 pad columns
            cm, sm = O.plan_mask(L, k + 1, "absent", N)
            lut, labels, _ = O.plan_ref(cm, sm)
            assert (lut[cm][per:] != 0).all() and (lut[cm][:per] == 0).sum() > 10
            cm, sm = O.plan_mask(L, 32, "slotless", N)
            lut, labels, _ = O.plan_ref(cm, sm)
            hc, hs = np.bincount(cm, minlength=256), np.bincount(sm, minlength=256)
            out = [l for l in range(256) if hc[l] and lut[l] == 255]
            assert len(out) == 2 and sorted(hc[out]) == [5, 11] and max(hs[out] / hc[out]) >= 100
            cm, _ = O.plan_mask(L, 1, "tile", N)
            assert (cm == cm[0]).all()
    for L in O.MASK_L:
        m = O.one_label_mask(L)
        assert (m == 7).sum() == 2 and not (m[64:128] == 0).any() and {0, 255} <= set(m.tolist())
        if L >= 1024:
            assert not (m[512:1024] == 0).any()
    for H, W, n, rect in O.CODE_LABEL_CASES:
        m = O.code_label_mask(H, W, n)
        lut, labels, _ = O.plan_ref(m, m)
        y, x = O.row_pixels(H, W, 2)
        rows, inside = m[y, x], O.rect_rows(H, W, 2, rect)
        assert len(labels) == n and all(((lut[rows] == s) & inside).sum() >= 2 for s in range(n)), (H, W, n, rect)


def test_row_pixels_is_a_bijection_and_rects_count():
    for sp, H, W, rect in O.CODE_CASES:
        y, x = O.row_pixels(H, W, sp)
        f = 2 if sp == 1 else 1
        assert len(set(zip(y.tolist(), x.tolist()))) == len(y) == H * W // (f * f) and y.max() == H // f - 1 and x.max() == W // f - 1
        if rect is not None:
            assert O.rect_rows(H, W, sp, rect).sum() == rect[2] * rect[3] // (f * f)
            assert sp == 2 or all(v % 2 == 0 for v in rect)


def test_packed_statistics_restatement():
    for sp, H, W, rect in O.CODE_CASES:
        N = 32 if sp == 2 else 128
        rows = O.code_rows(O.code_input(sp, H, W), H, W, sp)
        inside = O.rect_rows(H, W, sp, rect)
        L, per = O.code_groups(H, W, sp)
        want = O.stats64(rows.T, inside)
        r32 = O.stats32(np.ascontiguousarray(rows.T), inside.astype(np.uint8), 1, groups=(-(-L // per), per, "code"))
        e = O.stats_err(r32, want, N, skip=(O.CONST_CH,))
        print(f"stats_code sp={sp} {H}x{W} rect={rect}: e32 cov {e[0] / O.U:.3g} u, mean {e[1] / O.U:.3g} u")
        assert r32[0] == inside.sum() and e[0] < 1e-3


# ------------------------------------------------------------------------------------------------------------ factor
def test_factor_restatement_and_mutants():
    worst = {m: (0.0, None) for m in O.MUTANTS["factor"]}
    for N, k, ac, cond in O.FACTOR_CASES:
        content, styles, al = O.factor_input(N, k, cond)
        ev = np.linalg.eigvalsh(O.unpack(content, N)[2])
        assert 0.7 * cond < ev[-1] / ev[0] < 1.4 * cond                      # the condition number the case claims
        a32, info = O.factor32(content, styles, al, ac, N)
        assert info == [0] * (2 + k)
        ref = O.factor64(content, styles, al, ac, N, info)
        e32 = O.factor_err(a32, ref, N)
        print(f"factor N={N} styles={k} alpha_c={ac} cond={cond:g}: e32 {e32 / O.U:.3g} u")
        for m in O.MUTANTS["factor"][1:]:
            note(worst, m, O.ratio("factor", O.factor_err(O.factor32(content, styles, al, ac, N, mut=(m,))[0], ref, N), e32),
                 (N, k, ac, cond))
    for N in O.STATS_N:
        for kind in O.JITTER_KINDS:
            content = O.jitter_content(N, kind)
            _, styles, al = O.factor_input(N, 2, 10.0)
            trace = []
            a32, info = O.factor32(content, styles, al, 0.3, N, trace=trace)
            t = trace[-1]                                                    # the content's factorisation comes last
            margin = 100 * O.U * t["diag"]
            print(f"factor N={N} {kind}: tries {info}, last failed pivot {t['last_failed_pivot']:.3g}, smallest pivot of the "
                  f"successful try {t['min_pivot']:.3g}, margin {margin:.3g}")
            assert info[0] == {"rank_deficient": 2, "constant_channel": 1, "indefinite": 3}[kind] and info[1:] == [0, 0, 0]
            assert t["min_pivot"] >= margin
            # the failing pivot: 100 u away from zero, or a zero that no rounding can move (a zero row: every update is 0 * 0)
            assert t["last_failed_pivot"] <= -margin or (kind == "constant_channel" and t["last_failed_pivot"] == 0.0)
            ref = O.factor64(content, styles, al, 0.3, N, info)
            e32 = O.factor_err(a32, ref, N)
            got, info_m = O.factor32(content, styles, al, 0.3, N, mut=("jitter_not_cumulative",))
            note(worst, "jitter_not_cumulative", O.ratio("factor", O.factor_err(got, ref, N), e32), (N, kind, info_m))
            # the minimum-tries entry: starting from the count itself changes nothing, starting above it adds jitter
            assert O.factor32(content, styles, al, 0.3, N, min_tries=[info[0], 0, 0, 0])[1] == info
            assert O.factor32(content, styles, al, 0.3, N, min_tries=[info[0] + 2, 0, 1, 0])[1] == [info[0] + 2, 0, 1, 0]
    check_teeth("factor", worst, O.MUTANTS["factor"])


def test_prefactored_record_restates_bit_for_bit():
    N = 32
    content, styles, al = O.factor_input(N, 2, 1e4)
    L, tries = O.factor_chol32(styles[0], N, O.EPS)
    pre = O.pack(-(styles[0][0] + 1.0), O.unpack(styles[0], N)[1], L.astype(np.float64))
    a, _ = O.factor32(content, styles, al, 0.3, N)
    b, _ = O.factor32(content, [pre, styles[1]], al, 0.3, N)
    assert tries == 0 and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------- apply
def test_apply_restatement_and_mutants():
    worst = {m: (0.0, None) for m in O.MUTANTS["apply"]}
    worst_s = {m: (0.0, None) for m in O.MUTANTS["apply_split"] + O.MUTANTS["apply"]}
    claim = 0.0
    for N, L, prec, masked in O.APPLY_CASES:
        if masked:
            continue
        x, aff = O.apply_input(N, L)
        want, den = O.apply64(x, aff, N)
        split = O.apply_form(N, L, 0, 0, False, prec) == "split"
        op, fn, w = ("apply_split", O.apply_split32, worst_s) if split else ("apply", O.apply32, worst)
        r32 = fn(x, aff, N)
        e32 = O.apply_err(r32, want, den)
        print(f"{op} N={N} L={L}: e32 {e32 / O.U:.3g} u")
        if split:
            claim = max(claim, e32)
            assert e32 < O.SPLIT_CLAIM                                       # the emulated split under the header's own claim
        else:
            assert (r32[:, O.ZERO_PIXEL] == aff[N * N:]).all() and (r32[O.ZERO_ROW] == aff[N * N + O.ZERO_ROW]).all()
        for m in w:
            note(w, m, O.ratio(op, O.apply_err(fn(x, aff, N, mut=(m,)), want, den), e32), (N, L, prec))
    print(f"emulated split: at most {claim:.3g} of the claimed {O.SPLIT_CLAIM}")
    check_teeth("apply", worst, O.MUTANTS["apply"])
    check_teeth("apply_split", worst_s, list(worst_s))


def test_apply_labels_restatement_and_mutants():
    worst = {m: (0.0, None) for m in O.MUTANTS["apply_labels"]}
    for N, L, prec, n, ms, kind in O.APPLY_LABELS_CASES:
        if prec != "fp32" or L != 1092 or (N == 128 and n == 32 and kind != "runs"):
            continue
        x = O.apply_input(N, L, seed=5)[0]
        cm, sm = O.plan_mask(L, n, kind, N)
        lut, labels, _ = O.plan_ref(cm, sm)
        aff = O.affines_input(N, n)
        want, den = O.apply_labels_ref(x, aff, cm, lut, n, N, O.apply64, ms)
        r32 = O.apply_labels_ref(x, aff, cm, lut, n, N, O.apply32, ms)
        e32 = O.apply_err(r32, want, den)
        none = lut[cm] == 255
        assert r32[:, none].tobytes() == x[:, none].tobytes() and (kind != "slotless" or none.sum() == 16)
        for m in worst:
            got = O.apply_labels_ref(x, aff, cm, lut, n, N, O.apply32, ms, mut=(m,))
            note(worst, m, O.ratio("apply", O.apply_err(got, want, den), e32), (N, L, n, ms, kind))
    check_teeth("apply", worst, O.MUTANTS["apply_labels"])


# ------------------------------------------------------------------------------------------------------- composition
def test_references_compose_into_the_oracle():
    from oracle import cpu_ref
    N, H, W = 16, 12, 20
    g = torch.Generator().manual_seed(5)
    c, s = torch.randn(1, N, H, W, generator=g, dtype=torch.float64), torch.randn(1, N, H, W, generator=g, dtype=torch.float64) * 2 + 1
    want = cpu_ref.transfer(c, s)[0].reshape(N, -1).numpy()
    cx, sx = c[0].reshape(N, -1).numpy(), s[0].reshape(N, -1).numpy()
    T, t0, _, _ = O.factor64(O.stats64(cx), [O.stats64(sx)], [1.0], 0.0, N, [0, 0, 0])
    got = O.apply64(cx, np.concatenate([T.reshape(-1), t0]), N)[0]
    assert np.abs(got - want).max() < 1e-10 * np.abs(want).max()

    cm = (np.arange(H * W) % 3).astype(np.uint8).reshape(1, H, W)
    cm[0, 0, :4] = 9                                                         # a label without a slot
    sm = np.roll(cm, 7, axis=2)
    want = cpu_ref.transfer_seg(c, s, cm, sm)[0].reshape(N, -1).numpy()
    lut, labels, _ = O.plan_ref(cm, sm)
    assert labels == [0, 1, 2]
    affs = np.zeros((O.MAX_SLOTS, N * N + N))
    for k, lab in enumerate(labels):
        T, t0, _, _ = O.factor64(O.stats64(cx, cm.reshape(-1) == lab), [O.stats64(sx, sm.reshape(-1) == lab)], [1.0], 0.0, N, [0, 0, 0])
        affs[k] = np.concatenate([T.reshape(-1), t0])
    O.KAPP[N] = 8
    try:
        got = O.apply_labels_ref(cx, affs, cm.reshape(-1), lut, 3, N, O.apply64)[0]
    finally:
        del O.KAPP[N]
    assert np.abs(got - want).max() < 1e-10 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------- wrappers
def test_wrappers_call_what_the_header_declares():
    from vstnet_amd import _lib, cwct, cwct_ops
    assert cwct.ops is cwct_ops
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    src = open(os.path.join(REPO, "vstnet_amd", "cwct_ops.py")).read()
    used = set(re.findall(r"\bvst_[a-z0-9_]+", src)) - {"vst_cwct_apply"}
    assert used == set(NAMES), used ^ set(NAMES)
    L = built_library()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr) and name in _lib.EXPORTS, name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for fn in ("stats", "factor", "prefactor", "apply", "label_plan", "stats_labels", "factor_labels", "factor_labels_mix",
               "apply_labels", "stats_code", "stats_code_rect", "apply_code", "stats_labels_code", "stats_labels_code_rect",
               "apply_labels_code"):
        assert callable(getattr(cwct_ops, fn)), fn


def test_wrapper_refusals_need_no_gpu():
    from vstnet_amd import cwct_ops as ops
    x = torch.zeros(32, 68)
    plan = torch.zeros(2344, dtype=torch.uint8)
    for bad, msg in ((x.double(), "float32"), (x.t(), "contiguous"), (x[0], r"\[N, L\]"), (x, "CUDA"), (x[:, 1:65].contiguous()[:, 1:], "contiguous")):
        with pytest.raises(ValueError, match=msg):
            ops.stats(bad)
    assert x.reshape(-1)[4:4 + 32 * 16].view(32, 16).is_contiguous()         # a view at an element offset is what they accept
    with pytest.raises(ValueError, match="shape"):
        ops.stats(x, mask=torch.zeros(67, dtype=torch.uint8))
    with pytest.raises(ValueError, match="shape"):
        ops.apply(x, torch.zeros(32 * 32))
    with pytest.raises(ValueError, match="precision"):
        ops.apply(x.cpu(), torch.zeros(32 * 32 + 32), precision="fp16") if False else ops._prec("fp16")
    with pytest.raises(ValueError, match="float64"):
        ops.factor(torch.zeros(1 + 32 + 1024), [torch.zeros(1 + 32 + 1024)], [1.0], 32)
    with pytest.raises(ValueError, match="styles"):
        ops.factor(torch.zeros(1 + 32 + 1024, dtype=torch.float64), [], [], 32)
    with pytest.raises(ValueError, match="shape"):
        ops.stats_labels(x, torch.zeros(68, dtype=torch.uint8), plan[:100])
    with pytest.raises(ValueError, match="max_slots"):
        ops._slots(33)
    with pytest.raises(ValueError, match="floats"):
        ops.stats_code(torch.zeros(100), 8, 8, 2)
    with pytest.raises(ValueError, match="sp_steps"):
        ops.stats_code(torch.zeros(8 * 8 * 32), 8, 8, 3)
    with pytest.raises(ValueError, match="CUDA"):
        ops.apply_labels(x, torch.zeros(32, 32 * 32 + 32), torch.zeros(68, dtype=torch.uint8), plan)
    # the library's own refusals come before any launch
    import ctypes as C
    L = built_library()
    ok, null = C.c_void_p(4096), C.c_void_p(0)
    assert L.vst_cwct_stats(ok, 48, 64, null, 0, ok, ok, null) == -2 and L.vst_cwct_stats(ok, 32, 0, null, 0, ok, ok, null) == -1
    assert L.vst_cwct_stats(ok, 32, 64, null, 0, ok, null, null) == -4
    assert L.vst_cwct_apply_prec(ok, ok, 32, 64, ok, null, 0, 7, null) == -3
    assert L.vst_cwct_stats_code_rect(ok, 16, 16, 1, 1, 0, 2, 2, ok, ok, null) == -1      # artistic rows: odd origin
    assert L.vst_cwct_apply_labels_code(ok, ok, 8, 8, ok, ok, ok, 9, null) == -2
