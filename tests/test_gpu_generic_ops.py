"""csrc/generic.hip on the card, op by op through the C ABI: vst_generic_conv against the fp64 statement of
tests/generic_ref.py within the derived float32 running-error bound (n + 3) 2^-24 (S + |bias| + |old|), element by element, and
squeeze / unsqueeze / copy_channels / zero bit for bit, the grid-stride loop past the 65536-workgroup cap included.
tests/test_generic_host.py shows on the CPU that a dropped tap, a reflection off by one or exchanged ky / kx is hundreds to
thousands of times over the bound."""
import functools

import numpy as np
import pytest
import torch

import generic_ref as R
from zc import ptr, stream
from vstnet_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -7.0e30
GUARD = 64


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def want_conv(c):
    x, w, bias, old, sign = R.case_tensors(c)
    return R.conv(x, w, bias, c.K, c.stride, c.relu, old, sign)


def call_conv(L, x, w, bias, old, sign, relu, out, B, Cin, Cout, H, W, K, stride):
    return L.vst_generic_conv(ptr(x), ptr(w), ptr(bias) if bias is not None else None, ptr(old) if old is not None else None,
                              float(sign), int(relu), ptr(out), B, Cin, Cout, H, W, K, stride, stream())


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_conv_within_the_derived_bound(L, c):
    """|got - ref| <= (n + 3) 2^-24 (S + |bias| + |old|) on every element, n = 8 ceil(Cin / 8) K K.  The output buffer holds
    exactly B Cout Ho Wo elements and a guard behind them: the guard is intact and every element was written.  `old` may be the
    output buffer itself (vstnet.h: "out may alias old"): the alias cases give the same bits as the two-buffer call."""
    x, w, bias, old, sign = R.case_tensors(c)
    ref, bound = want_conv(c)
    n = ref.size
    out = torch.full((n + GUARD,), SENTINEL, device="cuda")
    d_old = None
    if c.old in ("plus", "minus"):
        d_old = dev(old)
    elif c.old:
        out[:n] = dev(old).reshape(-1)
        d_old = out
    _lib.check(call_conv(L, dev(x), dev(w), dev(bias), d_old, sign, c.relu, out, c.B, c.Cin, c.Cout, c.H, c.W, c.K, c.stride),
               "vst_generic_conv")
    got = out.cpu().numpy()
    assert (got[n:] == np.float32(SENTINEL)).all(), "guard written"
    got = got[:n].reshape(ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / bound).max())
    print(f"generic conv {R.case_id(c)}: worst error / bound {ratio:.3f}, max |err| {err.max():.3e}")
    assert (err <= bound).all(), (R.case_id(c), ratio)
    if c.old and c.old.startswith("alias"):
        out2 = torch.full((n,), SENTINEL, device="cuda")
        _lib.check(call_conv(L, dev(x), dev(w), dev(bias), dev(old), sign, c.relu, out2, c.B, c.Cin, c.Cout, c.H, c.W, c.K,
                             c.stride), "vst_generic_conv")
        assert np.array_equal(out2.cpu().numpy().view(np.uint32), got.reshape(-1).view(np.uint32))


def test_conv_refusals(L):
    x, w, bias = (torch.randn(s, device="cuda") for s in ((1, 2, 8, 8), (3, 2, 9, 9), (3,)))
    out = torch.full((3 * 8 * 8 + GUARD,), SENTINEL, device="cuda")
    call = lambda H, W, K, stride, b=bias: call_conv(L, x, w, b, None, 1.0, 0, out, 1, 2, 3, H, W, K, stride)
    for K in (0, 2, 4, 6, 8, 9):
        assert call(8, 8, K, 1) == -2, K
    assert call(8, 8, 3, 3) == -2 and call(8, 8, 3, 0) == -2
    assert call(1, 8, 3, 1) == -2 and call(8, 1, 3, 1) == -2           # H = pad: ReflectionPad2d needs pad < size
    assert call(3, 8, 7, 2) == -2 and call(2, 8, 5, 1) == -2
    assert call(8, 8, 3, 1, None) == -1
    assert L.vst_generic_conv(None, ptr(w), ptr(bias), None, 1.0, 0, ptr(out), 1, 2, 3, 8, 8, 3, 1, stream()) == -1
    assert L.vst_generic_conv(ptr(x), ptr(w), ptr(bias), None, 1.0, 0, None, 1, 2, 3, 8, 8, 3, 1, stream()) == -1
    assert L.vst_generic_conv(ptr(x), ptr(w), ptr(bias), None, 1.0, 0, ptr(out), 0, 2, 3, 8, 8, 3, 1, stream()) == -2
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("shape", R.SQUEEZE_SHAPES)
def test_squeeze_unsqueeze_exact(L, shape):
    B, D, H, W = shape
    x = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
    n = x.size
    y = torch.full((n + GUARD,), SENTINEL, device="cuda")
    _lib.check(L.vst_generic_squeeze(ptr(dev(x)), ptr(y), B, D, H, W, stream()), "vst_generic_squeeze")
    got = y.cpu().numpy()
    assert (got[n:] == np.float32(SENTINEL)).all()
    assert np.array_equal(got[:n].reshape(B, 4 * D, H // 2, W // 2), R.squeeze(x))
    back = torch.full((n + GUARD,), SENTINEL, device="cuda")
    _lib.check(L.vst_generic_unsqueeze(ptr(y), ptr(back), B, D, H, W, stream()), "vst_generic_unsqueeze")
    got = back.cpu().numpy()
    assert (got[n:] == np.float32(SENTINEL)).all()
    assert np.array_equal(got[:n].reshape(shape), x)                 # the round trip is the identity


def test_squeeze_refusals(L):
    x = torch.randn(1, 2, 6, 6, device="cuda")
    y = torch.full((72,), SENTINEL, device="cuda")
    for H, W in ((5, 6), (6, 5), (0, 6)):
        assert L.vst_generic_squeeze(ptr(x), ptr(y), 1, 2, H, W, stream()) == -2
        assert L.vst_generic_unsqueeze(ptr(x), ptr(y), 1, 2, H, W, stream()) == -2
    assert L.vst_generic_squeeze(None, ptr(y), 1, 2, 6, 6, stream()) == -1
    assert L.vst_generic_unsqueeze(ptr(x), None, 1, 2, 6, 6, stream()) == -1
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


@pytest.mark.parametrize("C_src,c0,n,C_dst,d0", R.COPY_CASES)
def test_copy_channels_exact(L, C_src, c0, n, C_dst, d0):
    B, H, W = 2, 3, 5
    src = np.random.default_rng(4).standard_normal((B, C_src, H, W)).astype(np.float32)
    dst0 = np.full((B, C_dst, H, W), SENTINEL, np.float32)
    dst = torch.full((dst0.size + GUARD,), SENTINEL, device="cuda")
    _lib.check(L.vst_generic_copy_channels(ptr(dev(src)), ptr(dst), B, C_src, c0, n, H * W, C_dst, d0, stream()), "copy_channels")
    got = dst.cpu().numpy()
    assert (got[dst0.size:] == np.float32(SENTINEL)).all()
    assert np.array_equal(got[:dst0.size].reshape(dst0.shape), R.copy_channels(src, dst0, c0, n, d0))


def test_copy_channels_refusals_and_zero(L):
    src = torch.randn(2, 5, 3, 5, device="cuda")
    dst = torch.full((2, 7, 3, 5), SENTINEL, device="cuda")
    call = lambda c0, n, d0, C_src=5, C_dst=7: L.vst_generic_copy_channels(ptr(src), ptr(dst), 2, C_src, c0, n, 15, C_dst, d0, stream())
    assert call(3, 3, 0) == -2 and call(0, 6, 0) == -2               # c0 + n > C_src
    assert call(0, 3, 5) == -2 and call(0, 5, 3) == -2               # d0 + n > C_dst
    assert call(-1, 2, 0) == -2 and call(0, 2, -1) == -2 and call(0, 0, 0) == -2
    assert L.vst_generic_copy_channels(None, ptr(dst), 2, 5, 0, 1, 15, 7, 0, stream()) == -1
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())
    flat = dst.view(-1)
    _lib.check(L.vst_generic_zero(ptr(flat[16:]), 100, stream()), "vst_generic_zero")
    got = flat.cpu().numpy()
    assert not got[16:116].view(np.uint32).any() and (got[:16] == np.float32(SENTINEL)).all() and (got[116:] == np.float32(SENTINEL)).all()
    assert L.vst_generic_zero(None, 4, stream()) == -1


# just over grid_for's cap of 65536 workgroups of 256: the only shapes at which the kernels' grid-stride loops take a second turn
BIG_H, BIG_W = 4098, 4096


def test_squeeze_past_the_grid_cap(L):
    assert BIG_H * BIG_W > 65536 * 256
    x = torch.randn(1, 1, BIG_H, BIG_W, device="cuda")
    y = torch.full((1, 4, BIG_H // 2, BIG_W // 2), SENTINEL, device="cuda")
    _lib.check(L.vst_generic_squeeze(ptr(x), ptr(y), 1, 1, BIG_H, BIG_W, stream()), "vst_generic_squeeze")
    want = x.reshape(1, 1, BIG_H // 2, 2, BIG_W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(1, 4, BIG_H // 2, BIG_W // 2)
    assert torch.equal(y, want)
    back = torch.full_like(x, SENTINEL)
    _lib.check(L.vst_generic_unsqueeze(ptr(y), ptr(back), 1, 1, BIG_H, BIG_W, stream()), "vst_generic_unsqueeze")
    assert torch.equal(back, x)


def test_copy_channels_past_the_grid_cap(L):
    B, HW = 2, BIG_H // 2 * BIG_W
    assert B * HW > 65536 * 256
    src = torch.randn(B, 2, HW, device="cuda")
    dst = torch.full((B, 2, HW), SENTINEL, device="cuda")
    _lib.check(L.vst_generic_copy_channels(ptr(src), ptr(dst), B, 2, 1, 1, HW, 2, 0, stream()), "copy_channels")
    assert torch.equal(dst[:, 0], src[:, 1]) and bool((dst[:, 1] == SENTINEL).all())
