"""The kernels of csrc/segformer.hip one by one (vstnet_amd.segformer.ops -> the kernel-level calls of include/vstnet.h, which
launch through the helpers a run uses) against fp64 references computed on the CPU at test time (tests/segformer_ops_ref.py).

Bounds.  e32 is torch's own op on the CPU in fp32 against the fp64 reference, at the same inputs under the same metric; the device
must stay within FACTOR_op x max(e32, floor_op).  FACTOR and the floors are constants of segformer_ops_ref.py, fixed on the host:
tests/test_segformer_ops_host.py shows that the fp32 restatement of the device arithmetic sits under FACTOR / 2 at every case
below and that a GEMM that loses one of its six products, a softmax that skips a rescale or the maximum, a LayerNorm with a
one-pass variance, no eps or the wrong divisor all exceed 1.25 x FACTOR at one of them.  im2col is a copy (bit equality); the RGB
gather is exact in the conv's zero padding and within 6 x 2^-24 x max(1, |want|) elsewhere.  Every output sits in a NaN-filled
buffer with a margin of a row and a column's worth on either side, which must stay NaN.  Every test prints its ratio (-s)
before it asserts; DESIGN.md section 5 ("The kernels one by one") has the table.

Measured on an MI355X: GEMM at most 1.14 of 3 (K = 1; 1.12 at K = 4096), LayerNorm 1.56 of 4, attention 1.10 of 4, dwconv +
GELU 1.00 of 8, head sum 1.94 of 8, RGB gather 3.55 u of 6 u.  The GEMM cases 65x64x4096 and 200x320x1280 without bias are the
ones that found seg_gemm_kernel's single accumulator chain (4.57 and 3.0007 x before it was split in three)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import segformer_ops_ref as O                                          # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vstnet_amd.segformer import ops
    return ops


def dev(*ts):
    return [None if t is None else t.cuda() for t in ts]


def d(*ts):
    return [None if t is None else t.double() for t in ts]


class Guarded:
    """A [rows][cols] fp32 output inside a NaN-filled buffer: a margin of one row and one column's worth (rows + cols floats,
    rounded up to the 16-byte grid) before and after it."""

    def __init__(self, rows, cols, fill=None):
        self.pad = (rows + cols + 3) // 4 * 4
        self.n = rows * cols
        self.buf = torch.full((self.n + 2 * self.pad,), float("nan"), dtype=torch.float32, device="cuda")
        self.out = self.buf[self.pad:self.pad + self.n].view(rows, cols)
        if fill is not None:
            self.out.copy_(fill)

    def check(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:self.pad]).all()) and bool(torch.isnan(self.buf[self.pad + self.n:]).all()), "margin written"
        return self.out.cpu()


def run_gemm(ops, a, w, bias, res, alias):
    g = Guarded(a.shape[0], w.shape[0], fill=res.cuda() if alias else None)
    da, dw, db, dr = dev(a, w, bias, None if alias else res)
    ops.gemm(da, dw, db, g.out if alias else dr, out=g.out)
    got = g.check()
    want = O.gemm(*d(a, w, bias, res))
    e32 = O.gemm_err(O.fp32(O.gemm, a, w, bias, res), want, a, w, bias, res)
    return got, want, O.ratio("gemm", O.gemm_err(got, want, a, w, bias, res), e32), e32


@pytest.mark.parametrize("variant", O.GEMM_VARIANTS, ids=lambda v: f"bias{int(v[0])}-res_{v[1]}")
@pytest.mark.parametrize("shape", O.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm(ops, shape, variant):
    a, w, bias, res = O.gemm_inputs(*shape)
    has_bias, res_mode = variant
    _, _, r, e32 = run_gemm(ops, a, w, bias if has_bias else None, None if res_mode == "none" else res, res_mode == "alias")
    print(f"gemm {shape} bias={has_bias} res={res_mode}: e32 {e32 / O.U:.2f} u, device {r:.2f} x max(e32, floor), bound {O.FACTOR['gemm']}")
    assert r <= O.FACTOR["gemm"], (shape, variant, r)


@pytest.mark.parametrize("name", O.GEMM_SPECIAL)
def test_gemm_special(ops, name):
    a, w = O.gemm_special(name)
    got, want, r, e32 = run_gemm(ops, a, w, None, None, False)
    print(f"gemm {name}: e32 {e32 / O.U:.2f} u, device {r:.2f} x max(e32, floor), bound {O.FACTOR['gemm']}")
    assert r <= O.FACTOR["gemm"], (name, r)
    if name == "zero rows":
        assert bool((got[want == 0] == 0).all()) and int((want == 0).sum()) == 4 * 70 + 2 * 70 - 8


@pytest.mark.parametrize("c,eps,inplace", O.LN_CASES)
def test_layernorm(ops, c, eps, inplace):
    x, g, b = O.layernorm_inputs(c)
    gd = Guarded(x.shape[0], c, fill=x.cuda() if inplace else None)
    dx, dg, db = dev(x, g, b)
    ops.layernorm(gd.out if inplace else dx, dg, db, eps, out=gd.out)
    got = gd.check()
    want = O.layernorm(*d(x, g, b), eps)
    r = O.token_ratio(got, O.fp32(O.layernorm, x, g, b, eps), want, O.layernorm_floor(x))
    print(f"layernorm C={c} eps={eps} inplace={inplace}: per token / u {np.round(O.token_errs(got, want) / O.U, 1)}, "
          f"device {r:.2f} x max(e32, floor) per token, bound {O.FACTOR['layernorm']}")
    assert r <= O.FACTOR["layernorm"], (c, eps, inplace, r)
    assert torch.equal(got[O.LN_ZERO_TOKEN], b)                      # an all-zero token gives b exactly


@pytest.mark.parametrize("case", O.AT_SHAPES + O.AT_SPECIAL, ids=lambda s: s.replace(" ", "_") if isinstance(s, str) else "x".join(map(str, s)))
def test_attention(ops, case):
    q, kv = O.attention_special(case) if isinstance(case, str) else O.attention_inputs(*case)
    n, c = q.shape
    g = Guarded(n, c)
    ops.attention(*dev(q, kv), O.AT_SCALE, out=g.out)
    got = g.check()                                                  # rows past N are not written
    want = O.attention(*d(q, kv), O.AT_SCALE)
    e32 = O.attention_err(O.fp32(O.attention, q, kv, O.AT_SCALE), want, kv)
    r = O.ratio("attention", O.attention_err(got, want, kv), e32)
    print(f"attention {case}: e32 {e32 / O.U:.2f} u, device {r:.2f} x max(e32, floor), bound {O.FACTOR['attention']}")
    assert bool(torch.isfinite(got).all())
    assert r <= O.FACTOR["attention"], (case, r)
    if kv.shape[0] == 1:
        assert torch.equal(got, kv[:, c:].expand(n, -1))             # one key: p = 1, l = 1, the V row bit for bit


@pytest.mark.parametrize("h,w,c", O.DW_CASES)
def test_dwconv_gelu(ops, h, w, c):
    x, wt, b = O.dwconv_inputs(h, w, c)
    g = Guarded(h * w, c)
    ops.dwconv_gelu(*dev(x, wt, b), h, w, out=g.out)
    got = g.check()
    want = O.dwconv_gelu(*d(x, wt, b), h, w)
    r = O.token_ratio(got, O.fp32(O.dwconv_gelu, x, wt, b, h, w), want, O.dwconv_floor(x, wt, b, h, w, want))
    print(f"dwconv+gelu {h}x{w} C={c}: worst token {O.token_errs(got, want).max() / O.U:.2f} u, device {r:.2f} x max(e32, floor) per token, "
          f"bound {O.FACTOR['dwconv_gelu']}")
    assert r <= O.FACTOR["dwconv_gelu"], (h, w, c, r)


@pytest.mark.parametrize("hi,wi,k,stride,pad,c", O.IM2COL_CASES)
def test_im2col_is_a_copy(ops, hi, wi, k, stride, pad, c):
    x = O.im2col_inputs(hi, wi, c)
    want = O.im2col(x, hi, wi, k, stride, pad)
    assert want.shape == (O.conv_out(hi, k, stride, pad) * O.conv_out(wi, k, stride, pad), k * k * c)
    g = Guarded(*want.shape)
    ops.im2col(x.cuda(), hi, wi, k, stride, pad, out=g.out)
    assert torch.equal(g.check(), want)


@pytest.mark.parametrize("h,w,chw", O.RGB_CASES)
def test_gather_rgb(ops, h, w, chw):
    frame = O.rgb_frame(h, w)
    want, pad = O.gather_rgb(frame)
    g = Guarded(*want.shape)
    ops.gather_rgb((frame.permute(2, 0, 1) if chw else frame).contiguous().cuda(), out=g.out)
    got = g.check()
    assert bool((got[pad] == 0).all()) and int(pad.sum()) > 0        # the conv's zero padding: exactly 0
    err = ((got.double() - want).abs() / want.abs().clamp(min=1.0))[~pad].max()
    print(f"gather_rgb {h}x{w} chw={chw}: {float(err) / O.U:.2f} u x max(1, |want|), allowed {O.RGB_TOL / O.U:.0f} u")
    assert float(err) <= O.RGB_TOL


@pytest.mark.parametrize("gi,alias", O.HEAD_CASES)
def test_head_sum(ops, gi, alias):
    grids, ys = O.HEAD_GRIDS[gi], O.head_inputs(gi)
    g = Guarded(*ys[0].shape, fill=ys[0].cuda() if alias else None)
    dys = dev(*ys)
    ops.head_sum([g.out if alias else dys[0]] + dys[1:], grids, out=g.out)
    got = g.check()
    want = O.head_sum(d(*ys), grids)
    r = O.token_ratio(got, O.fp32(O.head_sum, ys, grids), want, O.head_floor(ys, grids, want))
    print(f"head sum grids {grids} out_is_y0={alias}: device {r:.2f} x max(e32, floor) per token, bound {O.FACTOR['head_sum']}")
    assert r <= O.FACTOR["head_sum"], (gi, alias, r)
    assert float(got.min()) >= 0


def test_refusals_come_before_any_launch():
    """VST_E_ARG (-1): a null pointer, a float pointer off the 16-byte grid.  VST_E_SHAPE (-2): the documented conditions and
    non-positive sizes.  The output every call is given stays NaN."""
    from vstnet_amd import _lib
    L = _lib.lib()
    buf = torch.full((1 << 16,), float("nan"), dtype=torch.float32, device="cuda")
    inp = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    u8 = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    o, x, f, null = C.c_void_p(buf.data_ptr()), C.c_void_p(inp.data_ptr()), C.c_void_p(u8.data_ptr()), C.c_void_p(0)
    o4, x4 = C.c_void_p(buf.data_ptr() + 4), C.c_void_p(inp.data_ptr() + 4)
    hw8 = (C.c_int * 8)(18, 26, 9, 13, 5, 7, 3, 4)
    bad8 = (C.c_int * 8)(18, 26, 9, 13, 0, 7, 3, 4)
    ARG, SHAPE = -1, -2
    calls = [
        (ARG, L.vst_seg_gemm, (null, x, null, null, o, 8, 8, 8)), (ARG, L.vst_seg_gemm, (x, null, null, null, o, 8, 8, 8)),
        (ARG, L.vst_seg_gemm, (x, x, null, null, null, 8, 8, 8)), (ARG, L.vst_seg_gemm, (x4, x, null, null, o, 8, 8, 8)),
        (ARG, L.vst_seg_gemm, (x, x4, null, null, o, 8, 8, 8)), (ARG, L.vst_seg_gemm, (x, x, x4, null, o, 8, 8, 8)),
        (ARG, L.vst_seg_gemm, (x, x, null, x4, o, 8, 8, 8)), (ARG, L.vst_seg_gemm, (x, x, null, null, o4, 8, 8, 8)),
        (SHAPE, L.vst_seg_gemm, (x, x, null, null, o, 0, 8, 8)), (SHAPE, L.vst_seg_gemm, (x, x, null, null, o, 8, 0, 8)),
        (SHAPE, L.vst_seg_gemm, (x, x, null, null, o, 8, 8, 0)), (SHAPE, L.vst_seg_gemm, (x, x, null, null, o, -8, 8, 8)),
        (ARG, L.vst_seg_layernorm, (null, x, x, o, 5, 64, 1e-5)), (ARG, L.vst_seg_layernorm, (x, null, x, o, 5, 64, 1e-5)),
        (ARG, L.vst_seg_layernorm, (x, x, null, o, 5, 64, 1e-5)), (ARG, L.vst_seg_layernorm, (x, x, x, null, 5, 64, 1e-5)),
        (ARG, L.vst_seg_layernorm, (x, x, x, o4, 5, 64, 1e-5)), (ARG, L.vst_seg_layernorm, (x4, x, x, o, 5, 64, 1e-5)),
        (SHAPE, L.vst_seg_layernorm, (x, x, x, o, 5, 513, 1e-5)), (SHAPE, L.vst_seg_layernorm, (x, x, x, o, 5, 0, 1e-5)),
        (SHAPE, L.vst_seg_layernorm, (x, x, x, o, 0, 64, 1e-5)),
        (ARG, L.vst_seg_attention, (null, x, o, 8, 8, 64, 0.125)), (ARG, L.vst_seg_attention, (x, null, o, 8, 8, 64, 0.125)),
        (ARG, L.vst_seg_attention, (x, x, null, 8, 8, 64, 0.125)), (ARG, L.vst_seg_attention, (x, x4, o, 8, 8, 64, 0.125)),
        (SHAPE, L.vst_seg_attention, (x, x, o, 8, 8, 96, 0.125)), (SHAPE, L.vst_seg_attention, (x, x, o, 8, 8, 576, 0.125)),
        (SHAPE, L.vst_seg_attention, (x, x, o, 8, 8, 0, 0.125)), (SHAPE, L.vst_seg_attention, (x, x, o, 0, 8, 64, 0.125)),
        (SHAPE, L.vst_seg_attention, (x, x, o, 8, 0, 64, 0.125)),
        (ARG, L.vst_seg_dwconv_gelu, (null, x, x, o, 3, 5, 8)), (ARG, L.vst_seg_dwconv_gelu, (x, x, x4, o, 3, 5, 8)),
        (ARG, L.vst_seg_dwconv_gelu, (x, x, x, null, 3, 5, 8)),
        (SHAPE, L.vst_seg_dwconv_gelu, (x, x, x, o, 3, 5, 6)), (SHAPE, L.vst_seg_dwconv_gelu, (x, x, x, o, 0, 5, 8)),
        (SHAPE, L.vst_seg_dwconv_gelu, (x, x, x, o, 3, 5, 0)),
        (ARG, L.vst_seg_im2col, (null, 5, 7, 4, 2, 2, 0, o)), (ARG, L.vst_seg_im2col, (x, 5, 7, 4, 2, 2, 0, o4)),
        (SHAPE, L.vst_seg_im2col, (x, 5, 7, 6, 2, 2, 0, o)), (SHAPE, L.vst_seg_im2col, (x, 5, 7, 4, 0, 2, 0, o)),
        (SHAPE, L.vst_seg_im2col, (x, 5, 7, 4, 2, 0, 0, o)), (SHAPE, L.vst_seg_im2col, (x, 5, 7, 4, 2, 2, -1, o)),
        (SHAPE, L.vst_seg_im2col, (x, 5, 7, 4, 8, 8, 0, o)), (SHAPE, L.vst_seg_im2col, (x, 0, 7, 4, 2, 2, 0, o)),
        (ARG, L.vst_seg_gather_rgb, (null, 0, 72, 104, o)), (ARG, L.vst_seg_gather_rgb, (f, 0, 72, 104, null)),
        (ARG, L.vst_seg_gather_rgb, (f, 0, 72, 104, o4)),
        (SHAPE, L.vst_seg_gather_rgb, (f, 0, 0, 104, o)), (SHAPE, L.vst_seg_gather_rgb, (f, 1, 72, 31, o)),
        (ARG, L.vst_seg_head_sum, (null, x, x, x, hw8, 8, o)), (ARG, L.vst_seg_head_sum, (x, x, x4, x, hw8, 8, o)),
        (ARG, L.vst_seg_head_sum, (x, x, x, x, None, 8, o)), (ARG, L.vst_seg_head_sum, (x, x, x, x, hw8, 8, null)),
        (SHAPE, L.vst_seg_head_sum, (x, x, x, x, hw8, 6, o)), (SHAPE, L.vst_seg_head_sum, (x, x, x, x, hw8, 0, o)),
        (SHAPE, L.vst_seg_head_sum, (x, x, x, x, bad8, 8, o)),
    ]
    for k, (want, fn, args) in enumerate(calls):
        assert fn(*args, null) == want, (k, fn.__name__, want)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
