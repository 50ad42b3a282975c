"""The kernels of csrc/vgg.hip one by one (the kernel-level calls of include/vstnet.h), each against an exact yardstick:

  input      bit equality with the numpy float32 statement (tests/vgg_ref.py: input_f32)
  conv       bit equality with ReLU(vst_seg_gemm(col, W, bias)), col the reflect-gathered column matrix built on the host - the
             explicit route the implicit GEMM replaces - and the same outputs against an fp64 F.conv2d on the reflect-padded map
             under the GEMM's own bound (tests/segformer_ops_ref.py: FACTOR["gemm"], ratio, e32 from one thread)
  max-pool   bit equality with F.max_pool2d(ceil_mode=True)
  mean/std, MSE, loss   numpy fp64 within (n + 8) 2^-53 of the uncancelled sums, a bound that holds for ANY summation order:
             a sum of n terms in any order is off by at most (n - 1) 2^-53 sum |t|, the terms' own roundings (fp32 -> fp64 is
             exact, one subtraction, one product) and the final division and square root take the rest of the 8.  For the
             std the sum is the one under the root, sum (x - mean)^2 / (n - 1) + eps, and the bound goes through the root.

Every output sits in a NaN-filled buffer whose margins must stay NaN."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import segformer_ops_ref as O                                          # noqa: E402
import vgg_ref as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu
E53 = 2.0 ** -53


@pytest.fixture(scope="module")
def vgg():
    from vstnet_amd import vgg
    return vgg


def _seed(*ints):
    s = 777
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# -------------------------------------------------------------------------------------------------------------- input
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (9, 7)])
def test_input_kernels(vgg, hw):
    h, w = hw
    sd = R.weights()
    a, b = sd["0.weight"].reshape(3, 3), sd["0.bias"]
    img = R.image_u8(h, w, 5 + h)
    x3 = img.reshape(-1, 3).astype(np.float32) / np.float32(255)
    want = R.input_f32(x3, a.numpy(), b.numpy())
    got_u8 = vgg.input_map(torch.from_numpy(img).cuda(), a.reshape(9).cuda(), b.cuda()).cpu().numpy()
    planar = torch.from_numpy(np.ascontiguousarray(x3.T.reshape(3, h, w))).cuda()
    got_f32 = vgg.input_map(planar, a.reshape(9).cuda(), b.cuda()).cpu().numpy()
    assert got_u8.shape == (h * w, 4) and np.array_equal(got_u8.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got_f32.view(np.uint32), want.view(np.uint32))
    assert not got_u8[:, 3].any()


# --------------------------------------------------------------------------------------------------------------- conv
CONV_CASES = [(2, 2, 4, 64),          # both reflections of a pixel at once
              (3, 5, 64, 64),
              (9, 7, 64, 128),        # M = 63, one short of a tile
              (5, 13, 128, 72),       # M = 65, Cout not a tile multiple
              (2, 3, 512, 64)]        # K = 4608


def conv_inputs(h, w, cin, cout, clip):
    """a post-ReLU-like map (|randn|), weights of positive mean, so that the pre-activations are positive and a negative bias
    of their median clips half of them"""
    g = _seed(h, w, cin, cout)
    x = torch.randn((h * w, cin), generator=g).abs()
    wt = (torch.randn((cout, cin, 3, 3), generator=g) + 0.3) / float(9 * cin) ** 0.5
    bias = torch.randn(cout, generator=g)
    if clip:
        pre = R.reflect_col(x.double(), h, w) @ R.pack_weight(wt.double()).t()
        med = float(pre.median())
        assert med > 0.1
        bias = -med + 0.01 * bias
    return x, wt, bias


@pytest.mark.parametrize("clip", [False, True], ids=["bias", "clipping bias"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_is_the_explicit_route_bit_for_bit(vgg, case, clip):
    from vstnet_amd.segformer import ops
    h, w, cin, cout = case
    x, wt, bias = conv_inputs(h, w, cin, cout, clip)
    packed = R.pack_weight(wt)
    m = h * w
    pad = (m + cout + 3) // 4 * 4
    dx, dw, db = x.cuda(), packed.cuda(), bias.cuda()
    got = vgg.conv3x3_relu(dx, dw, db, h, w)
    explicit = torch.relu(ops.gemm(R.reflect_col(x, h, w).cuda(), dw, db))
    torch.cuda.synchronize()
    assert got.shape == (m, cout) and torch.equal(got, explicit), float((got - explicit).abs().max())
    assert bool((got.view(torch.int32) == explicit.view(torch.int32)).all())
    # a second call into a guarded buffer: nothing outside [M][Cout] is written, and the result is the same bits
    from vstnet_amd import _lib
    from vstnet_amd.resize import _ptr, _stream
    buf = torch.full((m * cout + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[pad:pad + m * cout]
    _lib.check(_lib.lib().vst_vgg_conv3x3_relu(_ptr(dx), _ptr(dw), _ptr(db), _ptr(out), h, w, cin, cout, _stream(None)), "conv")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + m * cout:]).all()), "margin written"
    assert torch.equal(out.view(m, cout), got)
    got = got.cpu()
    clipped = float((got == 0).float().mean())
    if clip:
        assert 0.3 < clipped < 0.7, clipped

    # against fp64 F.conv2d on the reflect-padded map, under the GEMM's own bound
    def conv(xx, ww, bb):
        mp = F.pad(xx.t().reshape(1, cin, h, w), (1, 1, 1, 1), mode="reflect")
        return R.tokens(torch.relu(F.conv2d(mp, ww, bb)))
    want = conv(x.double(), wt.double(), bias.double())
    col = R.reflect_col(x, h, w)
    e32 = O.gemm_err(O.fp32(conv, x, wt, bias), want, col, packed, bias)
    r = O.ratio("gemm", O.gemm_err(got, want, col, packed, bias), e32)
    print(f"conv {case} clip={clip}: clipped {clipped:.2f}, e32 {e32 / O.U:.2f} u, device {r:.2f} x max(e32, floor), bound {O.FACTOR['gemm']}")
    assert r <= O.FACTOR["gemm"], (case, clip, r)


# ----------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("c", [64, 4])
@pytest.mark.parametrize("hw", [(2, 2), (3, 3), (5, 4), (7, 9)])
def test_maxpool(vgg, hw, c):
    h, w = hw
    x = torch.randn((h * w, c), generator=_seed(h, w, c))
    want = R.tokens(F.max_pool2d(x.t().reshape(1, c, h, w), 2, 2, 0, ceil_mode=True))
    got = vgg.maxpool2(x.cuda(), h, w).cpu()
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("c", [5, 70])
@pytest.mark.parametrize("n", [4, 63, 4097])
def test_mean_std(vgg, n, c):
    x = torch.randn((n, c), generator=_seed(n, c))
    x[:, 1] = 100.0 + x[:, 1]                  # mean 100, deviation 1: a one-pass variance is off by 1e4 x this bound
    x[:, 2] = 0.0                              # a constant channel: std = sqrt(eps)
    got = vgg.mean_std(x.cuda(), R.EPS).cpu().numpy()
    v = x.numpy().astype(np.float64)
    mean = v.sum(axis=0) / n
    ss = ((v - mean) ** 2).sum(axis=0)
    var = ss / (n - 1)
    std = np.sqrt(var + R.EPS)
    bound_mean = (n + 8) * E53 * np.abs(v).sum(axis=0) / n
    # the sum under the root is q = sum d^2 / (n - 1) + eps, all terms positive: |dq| <= (n + 8) 2^-53 q, and d sqrt(q) =
    # dq / (2 sqrt(q)); the root's own rounding is inside the 8 (the sum's share of it is halved by the root)
    bound_std = (n + 8) * E53 * (var + R.EPS) / (2 * std)
    assert got.shape == (2, c)
    assert (np.abs(got[0] - mean) <= bound_mean).all(), float((np.abs(got[0] - mean) / np.maximum(bound_mean, 1e-300)).max())
    assert (np.abs(got[1] - std) <= bound_std).all(), float((np.abs(got[1] - std) / bound_std).max())
    assert got[0][2] == 0.0 and abs(got[1][2] - np.sqrt(R.EPS)) <= 2 * E53 * np.sqrt(R.EPS)
    assert abs(got[0][1] - 100.0) < 1.0 and abs(got[1][1] - 1.0) < 0.7


@pytest.mark.parametrize("n", [4, 63, 4097])
def test_mse(vgg, n):
    g = _seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) + 3.0
    got = float(vgg.mse_f64(a.cuda(), b.cuda()).cpu()[0])
    d2 = (a.numpy().astype(np.float64) - b.numpy().astype(np.float64)) ** 2
    want = d2.sum() / n
    assert abs(got - want) <= (n + 8) * E53 * d2.sum() / n, (got, want)
    assert float(vgg.mse_f64(a.cuda(), a.cuda()).cpu()[0]) == 0.0


def test_style_loss_of_records(vgg):
    g = _seed(11)
    ra, rb = torch.randn(1920, generator=g, dtype=torch.float64), torch.randn(1920, generator=g, dtype=torch.float64)
    got = float(vgg.style_loss_of_records(ra.cuda(), rb.cuda()).cpu()[0])
    want = float(R.loss_s_of(ra, rb))
    d2 = float(sum(((ra[o:o + 2 * c] - rb[o:o + 2 * c]) ** 2).sum() / c for o, c in zip(R.RECORD_OFFSETS, R.LEVEL_CHANNELS)))
    assert abs(got - want) <= (512 + 8) * E53 * d2, (got, want)
    assert float(vgg.style_loss_of_records(ra.cuda(), ra.cuda()).cpu()[0]) == 0.0
