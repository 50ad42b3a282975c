"""tests/generic_ref.py against torch and oracle/cpu_ref.py on the CPU, and the faults the card's bound must reject.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import generic_ref as R
from oracle import cpu_ref

T = torch.from_numpy


def test_case_list_covers_what_it_claims():
    ks = {(c.K, c.stride) for c in R.CASES}
    assert ks >= {(K, s) for K in (1, 3, 5, 7) for s in (1, 2)}
    assert {(c.Cin, c.Cout) for c in R.CASES} >= {(1, 1), (3, 9), (9, 2), (10, 17)}
    assert {(c.relu, c.old) for c in R.CASES} >= {(r, o) for r in (0, 1) for o in (None, "plus", "minus", "alias_plus", "alias_minus")}
    for K in (1, 3, 5, 7):                            # the smallest legal size of every K, both strides
        pad = (K - 1) // 2
        assert {c.stride for c in R.CASES if c.K == K and c.H == pad + 1 and c.W == pad + 1} == {1, 2}
    assert any(c.stride == 2 and c.H % 2 and c.W % 2 and c.B == 2 for c in R.CASES)
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_conv_reference_is_torch_fp64(c):
    x, w, bias, old, sign = R.case_tensors(c)
    ref, bound = R.conv(x, w, bias, c.K, c.stride, c.relu, old, sign)
    pad = (c.K - 1) // 2
    t = F.conv2d(F.pad(T(x).double(), (pad,) * 4, mode="reflect") if pad else T(x).double(), T(w).double(), T(bias).double(),
                 stride=c.stride)
    Ho, Wo = (c.H + 2 * pad - c.K) // c.stride + 1, (c.W + 2 * pad - c.K) // c.stride + 1
    assert tuple(t.shape) == ref.shape == (c.B, c.Cout, Ho, Wo)
    if c.relu:
        t = t.relu()
    if old is not None:
        t = T(old).double() + sign * t
    t = t.numpy()
    assert np.abs(ref - t).max() <= 1e-13 * max(np.abs(t).max(), 1.0)
    assert (bound > 0).all() and bound.shape == ref.shape
    # float32 torch is inside the bound too: the bound is not so tight that an honest float32 conv fails it
    t32 = F.conv2d(F.pad(T(x), (pad,) * 4, mode="reflect") if pad else T(x), T(w), T(bias), stride=c.stride)
    t32 = t32.relu() if c.relu else t32
    t32 = (T(old) + np.float32(sign) * t32) if old is not None else t32
    assert (np.abs(t32.numpy().astype(np.float64) - ref) <= bound).all()


@pytest.mark.parametrize("fault,floor", [("reflect", 1000), ("swap", 1000), ("tap", 100)])
def test_faults_are_far_over_the_bound(fault, floor):
    """a reflection off by one (2n - 1 - v) or ky / kx exchanged err by O(|w x|), thousands of times the bound, on every case they
    can touch (a 1 x 1 kernel has neither; a single output at stride 2 reads no row past the far edge); ONE dropped tap of up to
    49 per channel is still hundreds of times over it"""
    worst = {}
    for c in R.CASES:
        if c.K == 1 and fault != "tap":
            continue
        x, w, bias, old, sign = R.case_tensors(c)
        ref, bound = R.conv(x, w, bias, c.K, c.stride, c.relu, old, sign)
        bad, _ = R.conv(x, w, bias, c.K, c.stride, c.relu, old, sign, fault=fault)
        if np.array_equal(bad, ref):
            assert fault == "reflect" and c.stride == 2 and ref.shape[2:] == (1, 1), R.case_id(c)
            continue
        worst[R.case_id(c)] = float((np.abs(bad - ref) / bound).max())
    print(fault, "min over", len(worst), "cases of the worst error / bound:", min(worst.values()))
    assert len(worst) >= 30 and min(worst.values()) > floor, min(worst, key=worst.get)


@pytest.mark.parametrize("shape", R.SQUEEZE_SHAPES)
def test_squeeze_expressions_are_the_oracles(shape):
    x = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    y = R.squeeze(x)
    assert np.array_equal(y, cpu_ref.squeeze(T(x)).numpy())
    assert np.array_equal(R.unsqueeze(y), cpu_ref.unsqueeze(T(y)).numpy()) and np.array_equal(R.unsqueeze(y), x)
    B, D, H, W = shape
    b, d, h, w_, i, j = B - 1, D - 1, H // 2 - 1, 0, 1, 0           # one element through the sentence of the docstring
    assert y[b, (i * 2 + j) * D + d, h, w_] == x[b, d, 2 * h + i, 2 * w_ + j]


def test_copy_expressions_are_split_merge_and_inj_pad():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 6, 3, 5)).astype(np.float32)
    a, b = cpu_ref.split(T(x))
    n = 3
    z = np.full((2, 3, 3, 5), 9.0, np.float32)
    assert np.array_equal(R.copy_channels(x, z, 0, n, 0), a.numpy()) and np.array_equal(R.copy_channels(x, z, n, n, 0), b.numpy())
    m = R.copy_channels(b.numpy(), R.copy_channels(a.numpy(), np.zeros_like(x), 0, n, 0), 0, n, n)
    assert np.array_equal(m, cpu_ref.merge(a, b).numpy()) and np.array_equal(m, x)
    padded = R.copy_channels(x, np.zeros((2, 10, 3, 5), np.float32), 0, 6, 0)
    assert np.array_equal(padded, cpu_ref.inj_pad_fwd(T(x), 4).numpy())
    assert np.array_equal(R.copy_channels(padded, np.zeros_like(x), 0, 6, 0), cpu_ref.inj_pad_inv(T(padded), 4).numpy())
    for C_src, c0, n, C_dst, d0 in R.COPY_CASES:
        assert 0 <= c0 and c0 + n <= C_src and 0 <= d0 and d0 + n <= C_dst
    assert any(c0 == 0 for _, c0, _, _, _ in R.COPY_CASES) and any(c0 + n == C for C, c0, n, _, _ in R.COPY_CASES)
    assert any(d0 == 0 for *_, d0 in R.COPY_CASES) and any(d0 + n == C for _, _, n, C, d0 in R.COPY_CASES)
    assert any(n == 1 for _, _, n, _, _ in R.COPY_CASES) and any(n == C == Cd for C, _, n, Cd, _ in R.COPY_CASES)
