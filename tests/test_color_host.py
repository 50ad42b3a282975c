"""Host side of the Lab luminance blend's reference (tests/color_ref.py; no GPU): the float64 reference against its longdouble
twin and against the oracle, an fp32 emulation of the kernel under the reference's bound on every input set, planted faults in
that emulation failing the same comparison, and the conditions on the reference alone that make the comparison sharp (few
pixels near a knee, few values near a byte boundary, the gamut set clamped, the dark set not)."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import color_ref as R

SETS = ("uniform", "dark", "knees", "gamut", "bytes", "identity")
MODES = ("f32", "u8")


def test_float64_reference_against_its_longdouble_twin():
    """the reference's own rounding must be negligible against U = 2^-24: float64 rounds at 2^-53, the operations amplify
    that by the same conditioning the bound carries, so the deviation is asserted against 1e-6 of the fp32 bound and 1e-12"""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "this platform's longdouble is no wider than float64"
    for name in SETS:
        c, s, ref = R.case(name)
        v = ref.variants[0]
        wide = R.twin(c, s, ref.conds)
        dev = np.abs(wide - v.ref.astype(np.longdouble)).astype(np.float64)
        rel = float((dev / np.maximum(v.bound(), 1e-300)).max())
        print(f"{name}: float64 against longdouble, max deviation {dev.max():.3e}, at most {rel:.3e} of the fp32 bound")
        assert dev.max() <= 1e-12 and rel <= 1e-6


def test_reference_is_the_oracles_function():
    """oracle/cpu_ref.luminance_transfer (fp32 torch, mask-multiply selects) on `uniform`: within the bound plus the oracle's
    own error, which is of the same kind (fp32 roundings through the same conditioning, with torch's pow): the bound again."""
    c, s, ref = R.case("uniform")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.T.reshape(1, 3, 1, -1)))              # noqa: E731
    got = cpu_ref.luminance_transfer(t(c), t(s))[0, :, 0].numpy().T
    err = np.abs(got.astype(np.float64) - ref.ref)
    # the oracle selects by mask multiplication: pow(x) * 0 + lin * 1 adds nothing finite, so its selects are the reference's
    # except near a knee; allow the variants there
    ok = np.zeros(err.shape, bool)
    worst = np.full(err.shape, np.inf)
    for v in ref.variants:
        e = np.abs(got.astype(np.float64) - v.ref)
        b = 2.0 * v.bound() + 2.0 ** -23
        ok |= e <= b
        worst = np.minimum(worst, e / b)
    print(f"oracle against the reference on uniform: max abs {err.max():.3e}, worst error / (2 bound + 1 ulp) {worst.max():.3f}")
    assert ok.all()


@pytest.mark.parametrize("mode", MODES)
def test_emulation_passes_the_bound_on_every_set(mode):
    for name in SETS:
        c, s, ref = R.case(name, mode)
        out, conds = R.emulate(c, s)
        ok, worst, p_needed = R.check_float(out, ref)
        flips = sum(int((a != b).sum()) for a, b in zip(conds, ref.conds))
        okb, differ, maxd = R.check_bytes(R.quantise(out), ref)
        print(f"{name} ({mode}, {len(s)} pixels, {len(ref.variants)} variants): worst error / bound {worst:.3f}, P_needed "
              f"{p_needed:.3f}, selects taken the other way {flips}, bytes that differ {differ} (max {maxd})")
        assert ok.all() and worst <= 1.0
        assert okb.all() and maxd <= 1


FAULTS = [("g_y", "1.87599 -> 1.876"), ("zn_inv", "1.08883 -> 1.0888 where Z is rebuilt"),
          ("zn", "1.08883 -> 1.0888 where the stylised z is normalised"), ("finv_m", "7.787 -> 7.78 in lab_finv"),
          ("gamma", "exponent 2.4 -> 2.3999"), ("y_b", "0.072169 -> 0.07217"), ("no_zi_max", "fmaxf(0, .) on zi removed"),
          ("no_sty_clamp", "the stylised clamp removed"), ("L_from_stylised", "L from the stylised image"),
          ("swap_ab", "a and b swapped")]


@pytest.mark.parametrize("fault,what", FAULTS)
def test_planted_faults_fail_the_float_comparison(fault, what):
    caught = {}
    for name in SETS:
        c, s, ref = R.case(name)
        ok, worst, _ = R.check_float(R.emulate(c, s, fault)[0], ref)
        caught[name] = (int((~ok).sum()), worst)
    print(f"{what}: " + ", ".join(f"{k} {n} elements fail (worst {w:.3g})" for k, (n, w) in caught.items()))
    assert any(n > 0 for n, _ in caught.values()), what


def test_what_the_bound_resolves_of_powf():
    """a powf whose every result is off by k units of U * |z|, on top of numpy's own: k = 1 (the documented 1 ulp is 2 units at
    most) passes on every set, k = 8 fails on the sets of ordinary pixels.  That is the resolution P = 2 gives: DESIGN.md."""
    for k in (1.0, 2.0, 4.0, 8.0):
        row = {}
        for name in SETS:
            c, s, ref = R.case(name)
            ok, worst, p_needed = R.check_float(R.emulate(c, s, pow_off=k)[0], ref)
            row[name] = (int((~ok).sum()), worst, p_needed)
        print(f"powf off by {k:g} U|z|: " + ", ".join(f"{n} {f} fail (worst {w:.2f}, P_needed {p:.2f})" for n, (f, w, p) in row.items()))
        if k == 1.0:
            assert all(f == 0 for f, _, _ in row.values())
        if k == 8.0:
            assert all(row[n][0] > 0 for n in ("uniform", "gamut", "bytes", "identity"))


def test_planted_rounding_fails_the_byte_comparison():
    caught = {}
    for name in SETS:
        c, s, ref = R.case(name, "u8")
        out, _ = R.emulate(c, s)
        ok, _, _ = R.check_bytes(R.quantise(out, "round"), ref)
        assert R.check_bytes(R.quantise(out), ref)[0].all()
        caught[name] = int((~ok).sum())
    print("rounding instead of truncation: bytes that fail, " + ", ".join(f"{k} {n}" for k, n in caught.items()))
    # (identity with byte content puts every 255 * ref on an integer, where rounding gives the byte truncation should have)
    assert all(n > 0 for k, n in caught.items() if k != "identity")
    # ... and every constant or structural fault fails the byte comparison on some set too, far from any tolerance
    c, s, ref = R.case("uniform", "u8")
    for fault in ("swap_ab", "L_from_stylised", "no_sty_clamp"):
        assert not R.check_bytes(R.quantise(R.emulate(c, s, fault)[0]), ref)[0].all(), fault


@pytest.mark.parametrize("mode", MODES)
def test_conditions_on_the_reference_alone(mode):
    for name in SETS:
        c, s, ref = R.case(name, mode)
        v = ref.variants[0]
        any_near = np.zeros(len(s), bool)
        for k in R.KINDS:
            any_near |= ref.near[k]
        near_int, free = R.near_integer(v)
        clamped = float(1.0 - free.mean())
        share_int = float(near_int.sum() / max(int(free.sum()), 1))
        print(f"{name} ({mode}): near a knee {any_near.mean():.2e} of the pixels, 255 ref within its bound of an integer "
              f"{share_int:.2e} of the unclamped values, clamped {clamped:.3f}, median bound {np.median(v.bound()):.2e}")
        if name in ("uniform", "dark", "bytes"):
            assert any_near.mean() <= 1e-3
        if name != "knees" and (name, mode) != ("identity", "u8"):       # (bytes blended with themselves: 255 ref is the byte)
            assert share_int <= 1e-2
        if name == "gamut":
            assert clamped >= 0.20
        if name == "dark":
            assert float(v.ref.max()) < 1.0 and not (v.ref + v.bound() >= 1.0).any()
        assert np.isfinite(v.ref).all() and np.isfinite(v.bound()).all() and (v.bound() >= 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_knees_set_reaches_every_select(mode):
    """each select kind has pixels within the argument's bound of its threshold (for the sRGB decode, whose argument is exact:
    arguments on the threshold and on both sides within 8 ulps), and the fp32 emulation does take the other branch on some"""
    c, s, names = R.build_knees(mode)
    _, _, ref = R.case("knees", mode)
    args = R.select_args(R.content_of_bytes(c) if mode == "u8" else c, np.clip(s, 0, 1))
    thr = np.float32(R.K["srgb_knee"])
    lo, hi = R.neighbours(np.array([thr]), -8)[0], R.neighbours(np.array([thr]), 8)[0]
    calls = R.CALLS["srgb_s"] + (R.CALLS["srgb_c"] if mode == "f32" else ())
    for call in calls:
        a = args[call]
        assert (a == thr).any() and ((a > thr) & (a <= hi)).any() and ((a < thr) & (a >= lo)).any(), call
    for kind in ("lab_f", "lab_finv", "out"):
        n = int(ref.near[kind].sum())
        print(f"knees ({mode}): {n} of {len(s)} pixels within the bound of the {kind} threshold ({int((names == kind).sum())} built)")
        assert n >= 20, kind
    assert 2 <= len(ref.variants) <= 16
    _, conds = R.emulate(c, s)
    flips = sum(int((a != b).sum()) for a, b in zip(conds, ref.conds))
    print(f"knees ({mode}): the fp32 emulation takes {flips} selects the other way")
    assert flips > 0


def test_byte_entry_and_epilogue():
    b = np.arange(256, dtype=np.uint8)
    c = R.content_of_bytes(b)
    assert c.dtype == np.float32 and c[0] == 0 and c[255] == 1
    exact = b.astype(np.float64) / 255.0
    assert (np.abs(c.astype(np.float64) - exact) <= R.U * exact).all()                         # correctly rounded
    assert (c != (b.astype(np.float32) * np.float32(1.0 / 255.0))).any()                       # ... not a multiply by the reciprocal
    x = np.array([-0.1, 0.0, 0.5 / 255, 0.999 / 255, 1.0 / 255, 0.5, 254.999 / 255, 1.0, 1.2], np.float32)
    assert R.quantise(x).tolist() == [0, 0, 0, 0, 1, 127, 254, 255, 255]
