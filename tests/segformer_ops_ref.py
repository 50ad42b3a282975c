"""References, host restatements, mutants and the case generator of the per-kernel SegFormer tests (test infrastructure only;
tests/test_segformer_ops_host.py and tests/test_gpu_segformer_ops.py).

References: each op of csrc/segformer.hip from torch's own op, at the dtype of its inputs (fp64 = the truth, fp32 = e32, the
error an fp32 CPU run of the same op makes), with the device's token-major layout handled here.
Restatements: the device arithmetic restated in fp32 on the host (six-product split GEMM, chunked streaming softmax, two-pass
LayerNorm), each with switches that make it wrong in one way (the mutants): a bound that the restatement meets with room and
every mutant misses is a bound with teeth.
"""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from segformer_ref import MEAN, STD                                    # noqa: E402
from segformer_split_ratio import parts                               # noqa: E402

U = 2.0 ** -24                # unit roundoff of fp32
HEAD_DIM = 64
AT_KEYS = 16                  # keys per chunk of seg_attention_kernel

# ------------------------------------------------------------------------------------------------------------- bounds
# device error <= FACTOR x max(e32, floor), e32 = the fp32 CPU op against fp64 at the same inputs under the same metric.
# floor: storing the exact result in fp32 already costs up to u relative to the element, so an e32 under u (an fp32 op that
# happens to be exact at a tiny case: K = 1, an all-zero token, a 1 x 1 map) says nothing about what fp32 arithmetic can keep.
# The GEMM's denominator is sum |a w| + |bias| + |res| >= |out|, reached only at K = 1; its floor is half of u, which keeps the
# K = 4096 case's teeth (six products 0.3 u, a lost product 3.5 u and more, the bound 1.7 u there).
# The per-token ops (LayerNorm, dwconv + GELU, head sum) are compared TOKEN BY TOKEN (token_ratio): e32 and the floor are those
# of the token, so an ill-conditioned token (mean 100 / deviation 1: no fp32 LayerNorm is better than ~30 u there) does not lend
# its bound to the others.  There the floor is u x the token's condition - what rounding the op's own intermediates costs
# (layernorm_floor, dwconv_floor, head_floor) - and u itself on a well-conditioned token.
# FACTOR: the smallest round figure with restatement <= FACTOR / 2 at every case and every mutant >= 1.25 x FACTOR at one
# (tests/test_segformer_ops_host.py asserts both and prints the figures; DESIGN.md section 5 has the table).  GEMM: 3
# (restatement 0.4 - 1.1 x e32, any five products 4.7 x and more).  LayerNorm: 4 (restatement up to 1.95, mutants 40 x and more).
# Attention: 4 (restatement up to 1.1, mutants 1e4 x and more).  dwconv + GELU and the head sum take the 8 of
# tests/test_gpu_segformer.py: they fail grossly or not at all.
FACTOR = {"gemm": 3.0, "layernorm": 4.0, "attention": 4.0, "dwconv_gelu": 8.0, "head_sum": 8.0}
FLOOR = {"gemm": 0.5 * U, "layernorm": U, "attention": U, "dwconv_gelu": U, "head_sum": U}
RGB_TOL = 6 * U               # gather_rgb: |err| <= RGB_TOL x max(1, |want|); three roundings, the last divided by std >= 0.224,
                              # plus the fp32 mean / std constants


def ratio(op, err, e32):
    """err / max(e32, FLOOR): what FACTOR[op] bounds (GEMM, attention; the per-token ops use token_ratio)"""
    return err / max(e32, FLOOR[op])


# --------------------------------------------------------------------------------------------------------- references
@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def fp32(fn, *args):
    """fn(*args) on fp32 inputs with ONE CPU thread: e32.  torch's fp32 matmul sums K in blocks that follow the thread count, so
    e32 of a long-K GEMM otherwise moves from machine to machine (0.5 - 1.5 u at K = 4096), and the bound with it; the host test
    shows the mutants' teeth under the same e32 the device is held to."""
    with one_thread():
        return fn(*args)


def gemm(a, w, bias=None, res=None):
    y = F.linear(a, w, bias)
    return y if res is None else y + res


def layernorm(x, g, b, eps):
    return F.layer_norm(x, (x.shape[-1],), g, b, eps)


def attention(q, kv, scale):
    """q [N][C], kv [Nk][2C] with K of head h at column 64 h and V at C + 64 h -> [N][C]"""
    n, c = q.shape
    h = c // HEAD_DIM
    qh = q.reshape(n, h, HEAD_DIM).transpose(0, 1)
    k = kv[:, :c].reshape(-1, h, HEAD_DIM).transpose(0, 1)
    v = kv[:, c:].reshape(-1, h, HEAD_DIM).transpose(0, 1)
    a = torch.softmax((qh @ k.transpose(1, 2)) * scale, dim=-1)
    return (a @ v).transpose(0, 1).reshape(n, c)


def _planar(x, h, w):
    return x.t().reshape(1, x.shape[1], h, w)


def _tokens(m):
    return m.reshape(m.shape[1], -1).t()


def dwconv_gelu(x, w, b, h, wd):
    """x [h*wd][C], w [9][C] (tap-major), b [C]"""
    c = x.shape[1]
    y = F.conv2d(_planar(x, h, wd), w.t().reshape(c, 1, 3, 3), b, padding=1, groups=c)
    return F.gelu(_tokens(y))


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _unfold_rows(m, k, stride, pad):
    """F.unfold's [C*k*k][L] (c, ky, kx) -> rows [L][k*k*C] in the device's K order (ky, kx, c)"""
    c = m.shape[1]
    u = F.unfold(m, k, padding=pad, stride=stride)[0]
    return u.reshape(c, k * k, -1).permute(2, 1, 0).reshape(-1, k * k * c)


def im2col(x, hi, wi, k, stride, pad):
    return _unfold_rows(_planar(x, hi, wi), k, stride, pad)


def gather_rgb(frame_hwc_u8, dtype=torch.float64):
    """uint8 [H][W][3] -> (rows [T1][147] of patch_embed1's GEMM, mask of the taps in the conv's zero padding)"""
    f = frame_hwc_u8.permute(2, 0, 1)[None].to(dtype) / 255.0
    h, w = f.shape[2:]
    f = F.pad(f, (0, (4 - w % 4) % 4, 0, (4 - h % 4) % 4), mode="replicate")
    mean = torch.tensor(MEAN, dtype=dtype).reshape(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype).reshape(1, 3, 1, 1)
    rows = _unfold_rows((f - mean) / std, 7, 4, 3)
    inside = _unfold_rows(torch.ones_like(f), 7, 4, 3)
    return rows, inside == 0


def head_sum(ys, grids):
    """ys[i] [h_i*w_i][E] -> ReLU(y0 + sum_i upsample(y_i)) on grid 0, token-major"""
    acc = _planar(ys[0], *grids[0])
    for y, g in zip(ys[1:], grids[1:]):
        acc = acc + F.interpolate(_planar(y, *g), size=tuple(grids[0]), mode="bilinear", align_corners=False)
    return _tokens(F.relu(acc))


# ------------------------------------------------------------------------------------------------------------ metrics
def _np64(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def _ratio(err, den):
    """max err / den with 0 / 0 = 0, x / 0 = inf and NaN = inf"""
    err, den = np.nan_to_num(err, nan=np.inf, posinf=np.inf), np.broadcast_to(den, err.shape)
    out = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(out.max())


def gemm_err(got, want, a, w, bias=None, res=None):
    """componentwise: |err_ij| / (sum_k |a_ik w_jk| + |bias_j| + |res_ij|), max over the output (an absolute figure: x u)"""
    den = np.abs(_np64(a)) @ np.abs(_np64(w)).T
    if bias is not None:
        den = den + np.abs(_np64(bias))[None, :]
    if res is not None:
        den = den + np.abs(_np64(res))
    return _ratio(np.abs(_np64(got) - _np64(want)), den)


def token_errs(got, want):
    """per token max |err| / max |want| (a vector over the tokens)"""
    g, w = _np64(got), _np64(want)
    err, den = np.nan_to_num(np.abs(g - w).max(axis=1), nan=np.inf, posinf=np.inf), np.abs(w).max(axis=1)
    return np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))


def token_ratio(got, got32, want, floor_t):
    """max over the tokens of  err_t / max(e32_t, floor_t):  a token is held to the fp32 CPU op's error AT THAT TOKEN, so that
    one ill-conditioned token does not set the bound of the others.  floor_t (a vector, x u already applied) is what rounding
    the op's own intermediates to fp32 costs at that token; see the *_floor functions."""
    den = np.maximum(token_errs(got32, want), floor_t)
    return float((token_errs(got, want) / den).max())


def layernorm_floor(x):
    """The mean is a rounded fp32 number: off by up to u |mean|, which (x - mean) rstd g turns into u |mean| / max |x - mean| of
    the token's largest output.  A token of mean 100 and deviation 1 cannot be normalised to better than ~30 u in fp32."""
    x = _np64(x)
    mean = x.mean(axis=1)
    dev = np.abs(x - mean[:, None]).max(axis=1)
    return FLOOR["layernorm"] * (1.0 + np.abs(mean) / np.where(dev > 0, dev, 1.0))


def dwconv_floor(x, w, b, h, wd, want):
    """Every product and the bias are rounded against the pre-activation's magnitude sum |x||w| + |b|, and |GELU'| <= 1.13: a
    token whose outputs all sit in GELU's flat negative part is known only to u x that magnitude, not to u x its own size."""
    x, w, b = (torch.as_tensor(_np64(t)) for t in (x, w, b))
    c = x.shape[1]
    mag = _tokens(F.conv2d(_planar(x.abs(), h, wd), w.abs().t().reshape(c, 1, 3, 3), b.abs(), padding=1, groups=c))
    return FLOOR["dwconv_gelu"] * np.maximum(1.0, 1.13 * mag.numpy().max(axis=1) / np.maximum(np.abs(_np64(want)).max(axis=1), 1e-300))


def head_floor(ys, grids, want):
    """Every addend is rounded against its own size: a cell whose four addends cancel (or that the ReLU clips) is known only to
    u x (|y0| + sum up(|y_i|))."""
    mag = _planar(torch.as_tensor(_np64(ys[0])).abs(), *grids[0])
    for y, g in zip(ys[1:], grids[1:]):
        mag = mag + F.interpolate(_planar(torch.as_tensor(_np64(y)).abs(), *g), size=tuple(grids[0]), mode="bilinear", align_corners=False)
    mag = _tokens(mag).numpy().max(axis=1)
    return FLOOR["head_sum"] * np.maximum(1.0, mag / np.maximum(np.abs(_np64(want)).max(axis=1), 1e-300))


def attention_err(got, want, kv):
    """per query row and head max_d |err| / max |v| of that head, max over rows and heads"""
    g, w, kv = _np64(got), _np64(want), _np64(kv)
    n, c = w.shape
    h = c // HEAD_DIM
    err = np.abs(g - w).reshape(n, h, HEAD_DIM).max(axis=2)
    vmax = np.abs(kv[:, c:]).reshape(-1, h, HEAD_DIM).max(axis=(0, 2))
    return _ratio(err, vmax[None, :])


# ------------------------------------------------------------------------------------------- restatements and mutants
GEMM_MUTANTS = {"no lo.hi": (2, 0), "no hi.lo": (0, 2), "no mid.mid": (1, 1)}
LN_MUTANTS = ("one-pass variance", "eps ignored", "padded lane count")
AT_MUTANTS = ("acc not rescaled", "l not rescaled", "tail keys scored 0", "no max subtraction")


def gemm_restated(a, w, bias=None, res=None, mutant=None):
    """fp32: the six products of the three-way bf16 split, smallest first, then bias, then the residual"""
    pa, pw = parts(a.float(), 3), parts(w.float(), 3)
    drop = GEMM_MUTANTS[mutant] if mutant else None
    terms = sorted(((i + j, i, j) for i in range(3) for j in range(3) if i + j < 3), reverse=True)
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32)
    for _, i, j in terms:
        if (i, j) != drop:
            acc = acc + pa[i] @ pw[j].t()
    if bias is not None:
        acc = acc + bias.float()
    if res is not None:
        acc = acc + res.float()
    return acc


def _fma(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64; the sum is rounded to 53 bits and then to 24"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def layernorm_restated(x, g, b, eps, mutant=None):
    """fp32, one wave per token: lane l holds channels l, l + 64, ...; lane sums, a butterfly over the 64 lanes, two passes"""
    x, g, b = (t.float().numpy() for t in (x, g, b))
    t, c = x.shape
    f32 = np.float32
    live = (np.arange(512) < c).reshape(8, 64)
    v = np.zeros((t, 512), f32)
    v[:, :c] = x
    v = v.reshape(t, 8, 64)

    def wave_sum(p):
        s = np.zeros((t, 64), f32)
        for i in range(8):
            s = s + p[:, i]
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, np.arange(64) ^ o]
        return s[:, :1]
    n = f32(64 * ((c + 63) // 64) if mutant == "padded lane count" else c)
    mean = wave_sum(v) / n
    if mutant == "one-pass variance":
        var = wave_sum(v * v) / n - mean * mean
    else:
        d = np.where(live[None], v - mean[:, :, None], f32(0))
        var = wave_sum(d * d) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = f32(1) / np.sqrt(var + (f32(0) if mutant == "eps ignored" else f32(eps)))
        y = (v - mean[:, :, None]) * rstd[:, :, None]
    return torch.from_numpy(y.reshape(t, 512)[:, :c] * g + b)


def attention_restated(q, kv, scale, mutant=None):
    """fp32, a lane per query row and head: 16 keys per chunk, serial fmaf chains over d and over the keys, the running maximum
    m and sum l, `corr` = exp(m_old - m_new) on l and acc at every chunk, keys past Nk staged as zeros and scored -inf"""
    q, kv = q.float().numpy(), kv.float().numpy()
    n, c = q.shape
    nk = kv.shape[0]
    f32 = np.float32
    out = np.zeros((n, c), f32)
    for h in range(c // HEAD_DIM):
        qv = q[:, h * HEAD_DIM:(h + 1) * HEAD_DIM] * f32(scale)
        m, l, acc = np.full(n, -np.inf, f32), np.zeros(n, f32), np.zeros((n, HEAD_DIM), f32)
        for k0 in range(0, nk, AT_KEYS):
            live = min(nk - k0, AT_KEYS)
            kc, vc = np.zeros((AT_KEYS, HEAD_DIM), f32), np.zeros((AT_KEYS, HEAD_DIM), f32)
            kc[:live] = kv[k0:k0 + live, h * HEAD_DIM:(h + 1) * HEAD_DIM]
            vc[:live] = kv[k0:k0 + live, c + h * HEAD_DIM:c + (h + 1) * HEAD_DIM]
            s = np.zeros((n, AT_KEYS), f32)
            for d in range(HEAD_DIM):
                s = _fma(qv[:, d:d + 1], kc[None, :, d], s)
            if mutant != "tail keys scored 0":
                s[:, live:] = -np.inf
            with np.errstate(over="ignore", invalid="ignore"):
                if mutant == "no max subtraction":
                    mn, corr = m, np.ones(n, f32)
                    p = np.exp(s)
                else:
                    mn = np.maximum(m, s.max(axis=1))
                    corr = np.exp(m - mn)
                    p = np.exp(s - mn[:, None])
                if mutant != "l not rescaled":
                    l = l * corr
                if mutant != "acc not rescaled":
                    acc = acc * corr[:, None]
                for j in range(AT_KEYS):
                    l = l + p[:, j]
                    acc = _fma(p[:, j:j + 1], vc[j][None, :], acc)
            m = mn
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            out[:, h * HEAD_DIM:(h + 1) * HEAD_DIM] = acc * (f32(1) / l)[:, None]
    return torch.from_numpy(out)


# -------------------------------------------------------------------------------------------------------------- cases
def _seed(*ints):
    s = 12345
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


GEMM_SHAPES = [(64, 64, 32), (130, 150, 147), (65, 64, 36), (1, 1, 1), (64, 64, 8), (65, 70, 2048), (65, 64, 4096),
               (200, 320, 1280)]
GEMM_VARIANTS = [(bias, res) for bias in (False, True) for res in ("none", "separate", "alias")]
GEMM_SPECIAL = ["midlo", "zero rows"]


def gemm_inputs(m, n, k):
    """fp32 a [m][k] with rows scaled by exp(randn), w [n][k], bias [n], res [m][n]"""
    g = _seed(1, m, n, k)
    a = torch.randn((m, k), generator=g) * torch.exp(torch.randn((m, 1), generator=g))
    w = torch.randn((n, k), generator=g) / float(k) ** 0.5
    return a, w, torch.randn(n, generator=g), torch.randn((m, n), generator=g)


def gemm_special(name):
    """(a, w): "midlo" = a = 1 + j 2^-20 (j < 4096 at random) against w = +-1 alternating along k - the hi.hi products cancel and the result lives
    in the mid and lo parts of a; "zero rows" = whole zero rows of a and of w (their outputs are exactly 0)"""
    if name == "midlo":
        m, n, k = 33, 17, 4096
        j = torch.randint(0, 4096, (m, k), generator=_seed(9))
        a = 1.0 + j.float() * 2.0 ** -20
        w = (1.0 - 2.0 * ((torch.arange(k)[None, :] + torch.arange(n)[:, None]) % 2)).float()
        return a, w
    a, w, _, _ = gemm_inputs(70, 70, 64)
    a[[3, 64, 65, 66]] = 0
    w[[0, 69]] = 0
    return a, w


LN_CASES = [(c, eps, inplace) for c in (64, 128, 320, 512, 100) for eps in (1e-5, 1e-6) for inplace in (False, True)]
LN_ZERO_TOKEN = 3


def layernorm_inputs(c):
    """x [5][c]: randn; mean 100, std 1; variance about 1e-6 around 0.5; all zero; randn scaled by e^2.  g, b [c]"""
    g = _seed(2, c)
    x = torch.randn((5, c), generator=g)
    x[1] += 100.0
    x[2] = 0.5 + 1e-3 * x[2]
    x[LN_ZERO_TOKEN] = 0
    x[4] *= float(np.exp(2.0))
    return x, 1.0 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)


AT_SHAPES = [(130, 17, 128), (5, 1, 64), (128, 16, 64), (64, 99, 320), (12, 12, 512)]
AT_SPECIAL = ["peaked", "identical keys"]
AT_SCALE = 0.125


def attention_inputs(n, nk, c):
    """q = 2 randn, kv = randn: scores of standard deviation 2, so the running maximum rises in later chunks"""
    g = _seed(3, n, nk, c)
    return 2.0 * torch.randn((n, c), generator=g), torch.randn((nk, 2 * c), generator=g)


def attention_special(name):
    """"peaked": (64, 48, 64) with k_j = 8 e_j and q_i = the wanted score row, so score (i, j) = S[i][j] exactly, in [-90, 90]:
    rows 0-15 have their maximum (90) in chunk 0 (the running maximum never rises), 16-31 in chunk 1 over 50 in chunk 0 (rises
    once), 32-47 30 / 60 / 90 (rises at every chunk), 48-63 90 in chunk 0 and 90 - 2^-10 in chunk 2 (near-equal maxima).
    "identical keys": (20, 40, 64), every key the same, so the output is the mean of V."""
    g = _seed(4, len(name))
    if name == "identical keys":
        q, kv = attention_inputs(20, 40, 64)
        kv[:, :64] = kv[0, :64].clone()
        return q, kv
    n, nk, c = 64, 48, 64
    s = torch.rand((n, nk), generator=g) * 110.0 - 90.0                # [-90, 20)
    col = torch.randint(0, 16, (n,), generator=g)
    for i in range(n):
        grp, j = i // 16, int(col[i])
        if grp == 0:
            s[i, j] = 90.0
        elif grp == 1:
            s[i, j], s[i, 16 + j] = 50.0, 90.0
        elif grp == 2:
            s[i, j], s[i, 16 + j], s[i, 32 + j] = 30.0, 60.0, 90.0
        else:
            s[i, j], s[i, 32 + (j + 5) % 16] = 90.0, 90.0 - 2.0 ** -10
    q = torch.zeros((n, c))
    q[:, :nk] = s
    kv = torch.randn((nk, 2 * c), generator=g)
    kv[:, :c] = 0
    kv[torch.arange(nk), torch.arange(nk)] = 8.0
    return q, kv


DW_CASES = [(h, w, c) for (h, w) in ((1, 1), (1, 7), (7, 1), (3, 5)) for c in (8, 256)]


def dwconv_inputs(h, w, c):
    g = _seed(5, h, w, c)
    return 2.0 * torch.randn((h * w, c), generator=g), torch.randn((9, c), generator=g) / 3.0, torch.randn(c, generator=g)


IM2COL_CASES = [(hi, wi, k, s, p, c) for (hi, wi, k, s, p) in ((18, 26, 3, 2, 1), (17, 21, 3, 2, 1), (18, 26, 8, 8, 0), (5, 7, 2, 2, 0))
                for c in (4, 64)]


def im2col_inputs(hi, wi, c):
    return torch.randn((hi * wi, c), generator=_seed(6, hi, wi, c))


RGB_CASES = [(h, w, chw) for (h, w) in ((70, 101), (72, 104)) for chw in (0, 1)]


def rgb_frame(h, w):
    """uint8 [h][w][3]"""
    return torch.randint(0, 256, (h, w, 3), generator=_seed(7, h, w), dtype=torch.uint8)


HEAD_GRIDS = [((18, 26), (9, 13), (5, 7), (3, 4)), ((17, 21), (9, 11), (5, 6), (3, 3))]
HEAD_E = 8
HEAD_CASES = [(gi, alias) for gi in range(len(HEAD_GRIDS)) for alias in (False, True)]


def head_inputs(gi):
    g = _seed(8, gi)
    return [torch.randn((h * w, HEAD_E), generator=g) for h, w in HEAD_GRIDS[gi]]
