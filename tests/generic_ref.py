"""csrc/generic.hip restated in fp64 numpy: vst_generic_conv as a gather through explicit reflection indices and an einsum, with
the sum of absolute terms that prices the kernel's float32 accumulation, and the index expressions of squeeze / unsqueeze /
copy_channels.  tests/test_generic_host.py checks these against torch and oracle/cpu_ref.py on the CPU;
tests/test_gpu_generic_ops.py holds the card to them."""
import collections

import numpy as np

U = 2.0 ** -24                                         # float32 unit roundoff


def reflect(v, n, fault=False):
    """ReflectionPad2d index of coordinate v in [-(n-1), 2n-2]; fault=True is the off-by-one 2n - 1 - v on the far side"""
    v = np.abs(v)
    return np.where(v >= n, (2 * n - 1 if fault else 2 * n - 2) - v, v)


def out_size(n, K, stride):
    pad = (K - 1) // 2
    return (n + 2 * pad - K) // stride + 1


def conv(x, w, bias, K, stride, relu=0, old=None, sign=1.0, fault=None):
    """(ref, bound) in fp64.  ref = [old + sign *] [relu](conv(reflect_pad(x), w, stride) + bias); bound = the element-wise
    float32 running-error bound of the kernel (see conv_bound).  fault in (None, "reflect", "swap", "tap"): the planted faults
    of the host test (reflection off by one, ky / kx exchanged, the last tap dropped)."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    assert w.shape == (Cout, Cin, K, K)
    pad = (K - 1) // 2
    Ho, Wo = out_size(H, K, stride), out_size(W, K, stride)
    iy = reflect(np.arange(Ho)[:, None] * stride - pad + np.arange(K)[None, :], H, fault == "reflect")     # [Ho, K]
    ix = reflect(np.arange(Wo)[:, None] * stride - pad + np.arange(K)[None, :], W, fault == "reflect")     # [Wo, K]
    patches = x64[:, :, iy[:, None, :, None], ix[None, :, None, :]]                                        # [B, Cin, Ho, Wo, K, K]
    if fault == "swap":
        w64 = w64.transpose(0, 1, 3, 2)
    if fault == "tap":
        w64 = w64.copy()
        w64[:, :, K - 1, K - 1] = 0
    v = np.einsum("bchwyx,ocyx->bohw", patches, w64)
    S = np.einsum("bchwyx,ocyx->bohw", np.abs(patches), np.abs(w.astype(np.float64)))
    b64 = bias.astype(np.float64)[None, :, None, None]
    v = v + b64
    if relu:
        v = np.maximum(v, 0)
    o64 = np.zeros_like(v) if old is None else old.astype(np.float64)
    ref = v if old is None else o64 + sign * v
    return ref, conv_bound(S, np.abs(b64), np.abs(o64), Cin, K)


def conv_bound(S, abs_bias, abs_old, Cin, K):
    """The kernel adds n = 8 ceil(Cin / 8) K K float32 FMAs from zero in a fixed order (the zero-padded terms are exact), then
    the bias, then the ReLU (exact), then old + sign * v: n + 2 roundings at most, each relative to a partial sum that the sum S
    of the absolute terms (plus |bias|, |old|) bounds.  (n + 3) u (S + |bias| + |old|) leaves one u for the second-order
    terms, (1 + u)^(n+2) - 1 < (n + 3) u for every n here (n <= 784)."""
    n = 8 * ((Cin + 7) // 8) * K * K
    return (n + 3) * U * (S + abs_bias + abs_old)


Case = collections.namedtuple("Case", "B Cin Cout H W K stride relu old")    # old in (None, "plus", "minus", "alias_plus", "alias_minus")


def _cases():
    out = []
    olds = (None, "plus", "minus", "alias_plus", "alias_minus")
    n = 0

    def add(B, Cin, Cout, H, W, K, stride, relu=None, old=0):
        nonlocal n
        out.append(Case(B, Cin, Cout, H, W, K, stride, n & 1 if relu is None else relu, olds[n % 5] if old == 0 else old))
        n += 1

    # the smallest legal size, H = W = pad + 1: the reflection wraps on both sides inside one patch
    for K in (1, 3, 5, 7):
        for stride in (1, 2):
            for H, W in (((1, 1), (2, 3)) if K == 1 else (((K - 1) // 2 + 1,) * 2,)):
                add(1, 3, 5, H, W, K, stride)
    # output tiles that end mid-workgroup; the staged patch runs past the image
    for K in (3, 7):
        for stride in (1, 2):
            for H, W in ((17, 33), (31, 18)):
                add(1, 3, 9, H, W, K, stride)
    # channels off the 8-wide staging, B = 2, odd H and W (with stride 2: Ho = (H + 2 pad - K) // 2 + 1)
    for Cin, Cout in ((1, 1), (3, 9), (9, 2), (10, 17)):
        for K, stride in ((3, 2), (5, 1), (5, 2)):
            add(2, Cin, Cout, 9, 11, K, stride)
    # relu x old in full on one geometry
    for relu in (0, 1):
        for old in olds:
            add(2, 10, 17, 9, 11, 3, 1, relu, old)
    return tuple(out)


CASES = _cases()


def case_id(c):
    return f"B{c.B}_{c.Cin}to{c.Cout}_{c.H}x{c.W}_K{c.K}s{c.stride}_relu{c.relu}_{c.old or 'none'}"


def case_tensors(c):
    """(x, w, bias, old or None, sign) float32, seeded by the case"""
    rng = np.random.default_rng([c.B, c.Cin, c.Cout, c.H, c.W, c.K, c.stride])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    Ho, Wo = out_size(c.H, c.K, c.stride), out_size(c.W, c.K, c.stride)
    x, w, bias = f(c.B, c.Cin, c.H, c.W), f(c.Cout, c.Cin, c.K, c.K) / np.float32(np.sqrt(c.Cin) * c.K), f(c.Cout)
    old = 3 * f(c.B, c.Cout, Ho, Wo) if c.old else None
    sign = -1.0 if c.old in ("minus", "alias_minus") else 1.0
    return x, w, bias, old, sign


def squeeze(x):
    """y[b, (i 2 + j) D + d, h, w] = x[b, d, 2h + i, 2w + j]"""
    B, D, H, W = x.shape
    return np.ascontiguousarray(x.reshape(B, D, H // 2, 2, W // 2, 2).transpose(0, 3, 5, 1, 2, 4)).reshape(B, 4 * D, H // 2, W // 2)


def unsqueeze(y):
    B, C4, h, w = y.shape
    D = C4 // 4
    return np.ascontiguousarray(y.reshape(B, 2, 2, D, h, w).transpose(0, 3, 4, 1, 5, 2)).reshape(B, D, 2 * h, 2 * w)


def copy_channels(src, dst, c0, n, d0):
    """dst[b, d0 + k] = src[b, c0 + k], k < n; everything else of dst as it was"""
    out = dst.copy()
    out[:, d0:d0 + n] = src[:, c0:c0 + n]
    return out


SQUEEZE_SHAPES = ((1, 1, 2, 2), (2, 3, 6, 10), (1, 5, 34, 2))             # (B, D, H, W) of the unsqueezed tensor
# (C_src, c0, n, C_dst, d0): c0, d0 and n at both ends of their ranges
COPY_CASES = ((5, 0, 1, 7, 0), (5, 4, 1, 7, 6), (5, 0, 5, 7, 0), (5, 0, 5, 7, 2), (5, 2, 3, 3, 0), (1, 0, 1, 1, 0), (6, 1, 4, 9, 3))
