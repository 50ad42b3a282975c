"""tests/layout_ref.py against itself and against the library's host side, on the CPU: the packed-weight statement decoded
element by element through a loop written from the layout comment, the uint8 edge values, the normalisation seeds.  The last
group plants the faults the card's tests must catch and shows that the comparisons those tests make reject them.  No GPU."""
import numpy as np
import pytest

import layout_ref as R
import test_stage1_fold_host as fold
from vstnet_amd import _lib

F32 = np.float32


def sections_of(buf, cout, cin):
    """the sections of a packed buffer as arrays: f32 [9, cin, cout], the fragment sections [ksteps, 4, coutp, 8]"""
    L = R.pack_layout(cout, cin)
    shape = (L["ksteps"], 4, L["coutp"], 8)
    cut = lambda name: buf[L["sections"][name][0]:L["sections"][name][0] + L["sections"][name][1]]
    out = {"f32": np.frombuffer(cut("f32")[:L["f32_used"]], F32).reshape(9, cin, cout),
           "hi": R.bf16_value(np.frombuffer(cut("bf16_hi"), np.uint16)).reshape(shape),
           "lo": R.bf16_value(np.frombuffer(cut("bf16_lo"), np.uint16)).reshape(shape),
           "f16": np.frombuffer(cut("f16"), np.float16).reshape(shape)}
    if L["sections"]["f16_conv3"][1]:
        out["f16_conv3"] = np.frombuffer(cut("f16_conv3"), np.float16).reshape(shape)
    return out


def coords_loop(cin, ks, kg, j, conv3=False):
    """(tap, ci) of one fragment element, as the comment above pack_conv_kernel words it"""
    if cin >= 32:
        chunk, tap = divmod(ks, 9)
        k = kg * 8 + j
        if conv3:                                    # a producer lane's channels {4 kg + r, 16 + 4 kg + r}, r = j & 3
            k = 4 * kg + (j & 3) + (16 if j >= 4 else 0)
        return tap, chunk * 32 + k
    if cin == 16:
        return 2 * ks + (kg >> 1), (kg & 1) * 8 + j
    return 8 * ks + 2 * kg + (j >> 2), j & 3


@pytest.mark.parametrize("cout,cin", R.PACK_SHAPES)
def test_packed_conv_statement(cout, cin):
    w = R.pack_weights(cout, cin)
    assert np.abs(w).max() == 65504 and all((w == v).any() for v in R.PLANTED)
    buf = R.packed_conv(w)
    assert len(buf) == _lib.lib().vst_conv_packed_bytes(cout, cin) == R.pack_layout(cout, cin)["total"]
    s = sections_of(buf, cout, cin)
    assert np.array_equal(s["f32"], w.transpose(2, 3, 1, 0).reshape(9, cin, cout))
    L = R.pack_layout(cout, cin)
    assert ("f16_conv3" in s) == (cin >= 64 and cout >= 64)
    seen = np.zeros((cout, cin, 9), int)
    w9 = w.reshape(cout, cin, 9)
    with np.errstate(over="ignore"):
        for ks in range(L["ksteps"]):
            for kg in range(4):
                for j in range(8):
                    tap, ci = coords_loop(cin, ks, kg, j)
                    hi, lo, h = (s[n][ks, kg, :, j] for n in ("hi", "lo", "f16"))
                    if tap > 8 or ci >= cin:
                        assert not hi.any() and not lo.any() and not h.any()
                        continue
                    v = w9[:, ci, tap]
                    seen[:, ci, tap] += 1
                    assert not hi[cout:].any() and not lo[cout:].any() and not h[cout:].any()
                    # hi + lo holds 16 significant bits: each of the two roundings is within 2^-9 of its argument
                    assert (np.abs(hi[:cout].astype(np.float64) + lo[:cout] - v) <= 2.0 ** -16 * np.abs(v)).all()
                    assert np.array_equal(h[:cout], v.astype(np.float16))
                    if "f16_conv3" in s:
                        tap3, ci3 = coords_loop(cin, ks, kg, j, conv3=True)
                        assert np.array_equal(s["f16_conv3"][ks, kg, :cout, j], w9[:, ci3, tap3].astype(np.float16))
                        assert not s["f16_conv3"][ks, kg, cout:, j].any()
    assert (seen == 1).all()                         # every weight sits in the fragments exactly once


def test_cin16_items_are_the_fold_tests_items():
    """the one formula the suite already restated (test_stage1_fold_host.packed_items) and this statement agree"""
    w = R.pack_weights(fold.COUT, fold.CIN)
    assert np.array_equal(R.fragment_values(w), fold.packed_items(w.astype(np.float64)).astype(F32))


def test_rounding_statements():
    """bf16: ties to even both ways, on the bit pattern; the planted lo ties; fp16: the largest finite value and overflow"""
    b = lambda x: float(R.bf16_value(R.bf16_bits(np.array([x], F32)))[0])
    assert b(1 + 2.0 ** -8) == 1.0 and b(1 + 3 * 2.0 ** -8) == 1 + 2.0 ** -6 and b(-(1 + 2.0 ** -8)) == -1.0
    assert b(65504.0) == 65536.0 and b(2.0 ** -20) == 2.0 ** -20
    assert R.bf16_bits(np.array([-0.0], F32))[0] == 0x8000 and R.bf16_bits(np.array([0.0], F32))[0] == 0
    for v, lo_want in ((1 + 2.0 ** -10 + 2.0 ** -18, 2.0 ** -10), (1 + 2.0 ** -10 + 2.0 ** -17 + 2.0 ** -18, 2.0 ** -10 * (1 + 2.0 ** -6))):
        assert b(v) == 1.0 and b(F32(v) - F32(1.0)) == lo_want and float(F32(v) - F32(1.0)) != lo_want
    h = lambda x: R.f16_bits(np.array([x], F32)).view(np.float16)[0]
    assert h(65504.0) == 65504 and h(-65504.0) == -65504 and np.isposinf(h(70000.0)) and h(2.0 ** -20) == 2.0 ** -20
    # the planted values stay inside the fp32 normals and the fp16 normals-or-zero, 2^-20 apart (exact in fp16)
    p = np.abs(R.PLANTED[R.PLANTED != 0])
    assert (p >= 2.0 ** -20).all() and (p <= 65504).all()


@pytest.mark.parametrize("B,H,W", R.U8_SHAPES)
def test_u8_edge_statement(B, H, W):
    fr = R.u8_frames(B, H, W)
    if H * W >= 256:
        assert all(np.unique(fr[b, :, :, c]).size == 256 for b in range(B) for c in range(3))
    assert np.array_equal(R.unit_to_u8(R.u8_to_unit(np.arange(256, dtype=np.uint8))), np.arange(256))     # the edge round-trips
    v = R.u8_edge_values()
    planes = R.u8_edge_planes(B, H, W)
    held = set(planes.ravel().view(np.uint32).tolist())
    assert set(v[:9].view(np.uint32).tolist()) <= held
    if planes.size >= v.size:
        assert set(v.view(np.uint32).tolist()) == held
    q = R.unit_to_u8(v)
    assert q.dtype == np.uint8
    assert q[:9].tolist() == [0, 0, 0, 255, 255, 255, 255, 0, 0]
    k = np.arange(256)
    fam = q[9:].reshape(256, 3)
    assert np.array_equal(fam[:, 0], k) and np.array_equal(fam[:, 1], k)  # k / 255 and the float32 just above it: k
    below = fam[:, 2].astype(int) - k                                     # the float32 just below: k - 1 wherever the product
    assert set(below[1:].tolist()) <= {0, -1} and below[0] == 0           # rounds below k, which truncation must not hide
    assert (below == -1).sum() > 100, (below == -1).sum()


@pytest.mark.parametrize("cin1,mid,cout", R.NORM_CASES)
def test_normalize_seeds_have_no_row_near_a_half_integer(cin1, mid, cout):
    """the share of rows the card's test would have to leave out is zero for the committed seed, and the cases do what they are
    there for: both clamps act, the zero and Inf rows have scale 1, nothing turns NaN"""
    t = R.norm_tensors(cin1, mid, cout)
    out, scales, band = R.normalize_block(*t)
    assert band.sum() == 0
    assert not any(np.isnan(a).any() for a in out)
    e = -np.log2(scales.astype(np.float64))
    assert np.array_equal(e, np.round(e)) and np.abs(e).max() == 40
    if mid >= 4:
        assert e.max() == 40 and e.min() == -40
        assert scales[1] == 1 and scales[2] == 1 and scales[mid] == 1 and scales[mid + 3] == 1
        assert np.array_equal(out[0][2], t[0][2]) and np.isposinf(out[0][2]).sum() == 1
    # the rows phase 2 measures have the magnitudes the case chose: finite squares in float32
    mid_w4 = t[2] / scales[None, :mid, None, None]
    live = np.isfinite(mid_w4).all(axis=(1, 2, 3))
    assert (np.sum(mid_w4[live].astype(np.float64) ** 2, axis=(1, 2, 3)) < 2.0 ** 120).all()
    # live rows end with a norm in [2^-0.5, 2^0.5) unless a clamp acted
    for w, s in ((out[0], scales[:mid]), (out[2], scales[mid:])):
        lg = R.row_log2_norms(w)
        free = np.isfinite(lg) & (np.abs(np.log2(s.astype(np.float64))) < 40)
        assert (np.abs(lg[free]) <= 0.5).all()


# ------------------------------------------------------------------------------------------- the planted faults
def test_fault_lo_zeroed_is_seen_on_benign_weights():
    """unit normals, no planted value: a zero lo section changes bytes of that section alone, and would cost 2^-9 of a weight"""
    w = np.random.default_rng(5).standard_normal((16, 16, 3, 3)).astype(F32)
    want = R.packed_conv(w)
    o, n = R.pack_layout(16, 16)["sections"]["bf16_lo"]
    bad = want[:o] + bytes(n) + want[o + n:]
    assert R.packed_mismatches(want, want, 16, 16) == {}
    assert set(R.packed_mismatches(bad, want, 16, 16)) == {"bf16_lo"}


@pytest.mark.parametrize("cout,cin", [(4, 16), (64, 16)])
def test_fault_cin16_tap_order_swapped(cout, cin):
    """tap = 2 ks + (kg & 1), ci = 8 (kg >> 1) + j: the two bits of kg exchanged"""
    w = R.pack_weights(cout, cin)
    tap, ci = R.k_coords(cin, 5)
    swapped = (tap[:, [0, 2, 1, 3]], ci[:, [0, 2, 1, 3]])
    bad = b"".join(R.packed_sections(w, coords=swapped)[n] for n in R.SECTIONS)
    assert set(R.packed_mismatches(bad, R.packed_conv(w), cout, cin)) == {"bf16_hi", "bf16_lo", "f16"}


def test_unspecified_bytes_are_masked_and_nothing_else():
    cout, cin = 5, 32                                 # 5760 bytes of fp32, rounded to 5888
    w = R.pack_weights(cout, cin)
    want = bytearray(R.packed_conv(w))
    assert R.specified_mask(cout, cin).sum() == len(want) - 128
    for at in (5760, 5887):
        want[at] ^= 0xFF
    assert R.packed_mismatches(bytes(want), R.packed_conv(w), cout, cin) == {}
    want[5759] ^= 1
    want[5888] ^= 1
    assert R.packed_mismatches(bytes(want), R.packed_conv(w), cout, cin) == {"f32": 1, "bf16_hi": 1}


def test_fault_truncation_replaced_by_rounding():
    v = R.u8_edge_values()
    assert (R.unit_to_u8(v, rounding=True) != R.unit_to_u8(v)).sum() > 100
    planes = R.u8_edge_planes(1, 8, 8)                # even the smallest frame's sample tells the two apart
    assert (R.unit_to_u8(planes, rounding=True) != R.unit_to_u8(planes)).any()


@pytest.mark.parametrize("cin1,mid,cout", [c for c in R.NORM_CASES if c[1] >= 16])
def test_fault_scale_rounded_down(cin1, mid, cout):
    """floor(log2 norm) instead of round: about half of the unclamped rows get twice the scale, and the tensors follow (the
    cases with 1 and 4 rows are there for the clamps and the few-lanes paths; the two wide ones carry this)"""
    t = R.norm_tensors(cin1, mid, cout)
    out, scales, _ = R.normalize_block(*t)
    bad, bad_scales, _ = R.normalize_block(*t, round_down=True)
    assert (scales != bad_scales).sum() >= mid // 2
    assert not np.array_equal(out[2].view(np.uint32), bad[2].view(np.uint32))


def test_fault_wrong_w4_column():
    """W4's columns divided by the scale of row (i / 9) % mid: dividing by the row's own scale instead changes W4"""
    t = R.norm_tensors(64, 16, 64)
    out, scales, _ = R.normalize_block(*t)
    wrong = (t[2] / scales[:16, None, None, None])
    right = (t[2] / scales[None, :16, None, None])
    assert not np.array_equal(wrong.view(np.uint32), right.view(np.uint32))
