"""csrc/layout.hip on the card, kernel by kernel, against the exact statements of tests/layout_ref.py: vst_pack_conv byte for
byte over every section, the uint8 frame edge bit for bit on chosen values, vst_normalize_block's scales and tensors bit for bit.
Everything is called through the C ABI; tests/test_layout_host.py shows on the CPU which faults these comparisons reject."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import layout_ref as R
from zc import nchw_to_zc, zc_to_nchw, ptr, stream
from vstnet_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n_bytes, fill=0xA5):
    return torch.full((n_bytes + GUARD,), fill, dtype=torch.uint8, device="cuda")


@functools.lru_cache(maxsize=None)
def want_packed(cout, cin):
    w = R.pack_weights(cout, cin)
    return w, R.packed_conv(w)


# ------------------------------------------------------------------------------------------- vst_pack_conv
@pytest.mark.parametrize("cout,cin", R.PACK_SHAPES)
def test_pack_conv_bytes(L, cout, cin):
    """Every specified byte of the packed buffer equals the reference: the fp32 taps-major section, the bf16 hi and lo
    fragments, the fp16 fragments and, for cin, cout >= 64, conv3.hip's permuted-K fp16 fragments; the 256 guard bytes behind
    the buffer are intact.  The weights carry signed zeros, +-65504, bf16 ties in both directions (in hi and in lo) and 2^-20.
    Subnormal handling is not what this test is about: every planted value and every hi / lo term is an fp32 normal or zero, and
    the fp16 copies are normal, zero or (2^-20, small random weights) fp16 subnormals that both sides round as IEEE does."""
    w, want = want_packed(cout, cin)
    n = L.vst_conv_packed_bytes(cout, cin)
    assert n == len(want)
    buf = guarded(n)
    _lib.check(L.vst_pack_conv(ptr(dev(w)), cout, cin, ptr(buf), stream()), "vst_pack_conv")
    got = buf.cpu().numpy()
    assert (got[n:] == 0xA5).all(), "guard bytes written"
    assert R.packed_mismatches(got[:n].tobytes(), want, cout, cin) == {}


def test_pack_conv_refusals(L):
    w = dev(R.pack_weights(16, 16))
    buf = guarded(1 << 16)
    for cin in (8, 48):
        assert L.vst_pack_conv(ptr(w), 16, cin, ptr(buf), stream()) == -2
    assert L.vst_pack_conv(ptr(w), 0, 16, ptr(buf), stream()) == -1
    assert L.vst_pack_conv(None, 16, 16, ptr(buf), stream()) == -1
    assert L.vst_pack_conv(ptr(w), 16, 16, None, stream()) == -1
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())


def test_pack_conv_weight_range_flag(L):
    """|w| = 65504 exactly is the largest weight that fits fp16: RANGE_WEIGHT stays clear; one 70000 raises it and its fp16
    item is +Inf (the bf16 and fp32 sections hold it as they hold any value)"""
    cout, cin = 16, 16
    w, want = want_packed(cout, cin)
    n = len(want)
    _lib.range_flags(reset=True)
    try:
        buf = guarded(n)
        _lib.check(L.vst_pack_conv(ptr(dev(w)), cout, cin, ptr(buf), stream()), "vst_pack_conv")
        assert _lib.range_flags() & _lib.RANGE_WEIGHT == 0
        w2 = w.copy()
        at = np.flatnonzero(w2.reshape(-1) == np.float32(1 + 2.0 ** -8))[0]
        w2.reshape(-1)[at] = 70000.0
        _lib.check(L.vst_pack_conv(ptr(dev(w2)), cout, cin, ptr(buf), stream()), "vst_pack_conv")
        assert _lib.range_flags() & _lib.RANGE_WEIGHT
        got = buf.cpu().numpy()[:n].tobytes()
        assert R.packed_mismatches(got, R.packed_conv(w2), cout, cin) == {}
        o, ln = R.pack_layout(cout, cin)["sections"]["f16"]
        f16 = np.frombuffer(got[o:o + ln], np.float16)
        assert np.isposinf(f16).sum() == 1 and not np.isneginf(f16).any()
        assert _lib.range_flags(reset=True) & _lib.RANGE_WEIGHT and _lib.range_flags() == 0
    finally:
        _lib.range_flags(reset=True)                 # no other test inherits the flag


# ------------------------------------------------------------------------------------------- uint8 frame edge
@pytest.mark.parametrize("B,H,W", R.U8_SHAPES)
def test_pack_input_u8_exact(L, B, H, W):
    """channels 0..2 of s1 are float32(u8) / float32(255), a true division; channels 3..15 and all of s2 are exactly zero"""
    fr = R.u8_frames(B, H, W)
    s1 = torch.full((B, H // 4, W // 4, 256), 7.0, device="cuda")
    s2 = torch.full_like(s1, 7.0)
    _lib.check(L.vst_pack_input_u8(ptr(dev(fr)), ptr(s1), ptr(s2), B, H, W, stream()), "vst_pack_input_u8")
    x = zc_to_nchw(s1.cpu(), 16).numpy()
    want = R.u8_to_unit(fr).transpose(0, 3, 1, 2)
    assert np.array_equal(x[:, :3].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert not x[:, 3:].view(np.uint32).any()
    assert not s2.cpu().numpy().view(np.uint32).any()


@pytest.mark.parametrize("B,H,W", R.U8_SHAPES)
def test_unpack_output_u8_exact(L, B, H, W):
    """trunc(clip(float32(x) * float32(255), 0, 255)) with NaN -> 0, on k / 255 and its float32 neighbours for every k, -0.0,
    small and large negatives, 1, the float32 above 1, 7.5, +-Inf and NaN; channels 3..15 hold 1e30 and must not leak.  With
    VST_OPT_OUT_RGB = 1 (the default) vst_revnet_inverse_u8 writes the bytes from its last block's epilogue and never launches
    this kernel, so the whole-net tests do not reach it: hence a test of its own."""
    planes = R.u8_edge_planes(B, H, W)
    x = np.full((B, 16, H, W), 1e30, np.float32)
    x[:, :3] = planes
    s1 = nchw_to_zc(torch.from_numpy(x)).cuda()
    n = B * H * W * 3
    out = guarded(n, 0x5A)
    _lib.check(L.vst_unpack_output_u8(ptr(s1), ptr(out), B, H, W, stream()), "vst_unpack_output_u8")
    got = out.cpu().numpy()
    assert (got[n:] == 0x5A).all(), "guard bytes written"
    want = R.unit_to_u8(planes).transpose(0, 2, 3, 1)
    bad = np.argwhere(got[:n].reshape(B, H, W, 3) != want)
    assert bad.size == 0, [(tuple(i), float(planes[i[0], i[3], i[1], i[2]]), int(got[:n].reshape(B, H, W, 3)[tuple(i)]),
                            int(want[tuple(i)])) for i in bad[:8]]


# ------------------------------------------------------------------------------------------- vst_normalize_block
@pytest.mark.parametrize("cin1,mid,cout", R.NORM_CASES)
def test_normalize_block_exact(L, cin1, mid, cout):
    """scales and all five tensors bit-equal to the restatement (fp64 row norms, round(log2), clamp to +-40, 1 for a zero or
    non-finite norm).  No row of these seeds has log2 of its norm within 1e-4 of a half-integer (asserted on the CPU in
    test_layout_host.py), so the float32 summation order of the device cannot change a scale and nothing is left out."""
    t = R.norm_tensors(cin1, mid, cout)
    want, want_scales, band = R.normalize_block(*t)
    assert not band.any()
    d = [dev(a) for a in t]
    sc = torch.full((2 * mid + 8,), -5.0, device="cuda")
    _lib.check(L.vst_normalize_block(*(ptr(a) for a in d), cin1, mid, cout, ptr(sc), stream()), "vst_normalize_block")
    got_scales = sc.cpu().numpy()
    assert (got_scales[2 * mid:] == -5.0).all()
    assert np.array_equal(got_scales[:2 * mid].view(np.uint32), want_scales.view(np.uint32)), \
        np.flatnonzero(got_scales[:2 * mid] != want_scales)
    for name, g, w_ in zip(("w1", "b1", "w4", "b4", "w7"), d, want):
        g = g.cpu().numpy()
        assert not np.isnan(g).any(), name
        assert np.array_equal(g.view(np.uint32), w_.view(np.uint32)), (name, int((g.view(np.uint32) != w_.view(np.uint32)).sum()))
    # scales are optional: the same tensors without them
    d2 = [dev(a) for a in t]
    _lib.check(L.vst_normalize_block(*(ptr(a) for a in d2), cin1, mid, cout, None, stream()), "vst_normalize_block")
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(d, d2))
