"""How one coupling block is tested on its own (helper, no tests in it): tests/test_gpu_block_tiles.py runs it on the card,
tests/test_block_bounds_host.py proves on the CPU that the bound rejects what it is meant to catch.

The block is called through vst_block_apply with dst = 0, so that what comes back is +F(src) (direction +1) or -F(src)
(direction -1) and no state dilutes the error of F.  Two fp64 references, both oracle/cpu_ref.py's residual_F on fp64 copies:

  F64 of the exact weights                     for bf16x3 and for fp32 (the diagnostic direct conv),
  F64 of emul.rounded_weights (fp16, once)     for f16x2 and f16x2h: the pack-time exponent normalisation scales by powers of
                                               two, so these are the fp16 weights the kernels multiply with.

Bound per case and mode, for rel-L2 and max-rel alike (tests/zc.py's rel_err: of ||F|| and of max |F|):

  bound = 2 x (model_error + e32)

  model_error  tests/emul.py's model of the mode, evaluated in fp64, against the mode's reference: the error of the operand
               roundings alone (bf16x3: 16-bit hi + lo operands; f16x2: 22-bit inputs; f16x2h: single-fp16 h1 / h2).  0 for fp32.
  e32          the oracle's float32 residual_F against F64 of the exact weights: the price of float32 accumulation in some order.
  2            for what the model does not carry: bf16x3 keeps a_lo w_lo, which the kernels drop (2^-18 per product), and the
               MFMA summation order is not the oracle's.

None of these figures comes from the kernels.

MODEL CORRECTION (fp32).  With model_error = 0 for the diagnostic direct conv, i.e. a bound of 2 x e32, the 256-channel blocks
landed at 3.0 x e32 (9e-7 of F against e32 = 3e-7) at every shape alike, the stride-2 one at 2.0, the 64-channel stride-1 block
at 1.6.  That is arithmetic, not a fault: conv_fp32_kernel (vstnet_amd/csrc/conv.hip) keeps ONE accumulator per output,
`float acc = a.bias[co]` followed by `acc = fmaf(p[ci], w[(size_t)ci * COUT], acc)` over 9 taps x CIN channels - a serial chain
of up to 2304 float32 additions, whose rounding error grows with the chain's length - while e32 is the oracle's blocked
summation.  "float32 accumulation in some order" underprices that one order, so the fp32 mode gets a model like the others: the
same chain, evaluated on the CPU (_conv_chain32).  It loosens the fp32 bound from 2 x e32 to 2 x (chain + e32), about 2.4e-6 of
F for the 256-channel blocks and 1.3e-6 for the 16-channel one - still five times under the bf16x3 bound.  No MFMA mode is touched.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import emul
from tests.zc import nchw_to_zc, zc_to_nchw, ptr, stream, rel_err

# (name, index in the packed block list, state-dict prefix, channel, stride): the six of tests/test_gpu_parity.py's BLOCKS
BLOCKS = [("c16s1", 3, "stack.3.", 16, 1), ("c64s2", 10, "stack.10.", 64, 2), ("c64s1", 13, "stack.13.", 64, 1),
          ("c256s2", 20, "stack.20.", 256, 2), ("c256s1", 25, "stack.25.", 256, 1),
          ("cr0", 30, "channel_reduction.block_list.0.", 256, 1)]
MODES = ("fp32", "bf16x3", "f16x2", "f16x2h")
SENTINEL = 12345.0

# Shapes, rows x cols at the level where the block's convs write (h x w); the frame of the call is that << level.
#   20 x 36, B = 3  an interior seam and a 4-wide ragged edge in both axes: 2 x 3 tiles of 16 x 16 (3 x 3 of the 8-row tiles of the
#                   stride-2 convs and the lean stage-3 form), 18 / 27 tiles (xcd_tile with per = 3 / 4, idle tail workgroups in
#                   the grid rounded up to 8), images 1 and 2 of a batch
#   32 x 16, B = 1  exact multiples of the tile
#   the smallest legal extent of the level beside a second tile as narrow as the level allows (frames are multiples of 4, >= 8):
#                   level 2: 2 x 18 / 18 x 2 (reflection folds a 2-pixel axis; a 2-wide last tile), level 1: 4 x 18 / 18 x 4,
#                   level 0: 8 x 20 / 20 x 8 (a 4-wide last tile), B = 2
#   frame 68 x 132, B = 1: a last tile as thin as the level allows.  Frames are multiples of 4 (vst_shape_ok), so a level-2 view
#                   can be odd - 17 x 33, a last tile of one row and one column - and a level-1 view is even: 34 x 66, a last tile
#                   of 2 x 2.  (A level-0 view is the frame: its ragged 4 is in 20 x 36.)
_SHAPES = {
    16: [(20, 36, 3), (32, 16, 1), (8, 20, 2), (20, 8, 2)],
    64: [(20, 36, 3), (32, 16, 1), (4, 18, 2), (18, 4, 2), (34, 66, 1)],
    256: [(20, 36, 3), (32, 16, 1), (2, 18, 2), (18, 2, 2), (17, 33, 1)],
}


@dataclass(frozen=True)
class Case:
    name: str
    k: int
    prefix: str
    channel: int
    stride: int
    h: int
    w: int
    B: int

    @property
    def level(self):
        return {16: 0, 64: 1, 256: 2}[self.channel]

    @property
    def frame(self):
        return self.h << self.level, self.w << self.level

    @property
    def src_shape(self):
        """F's input as an NCHW view: the block's own level, or the finer one (a quarter of the channels) for stride 2"""
        s = self.stride
        return self.B, self.channel // (s * s), self.h * s, self.w * s

    @property
    def seed(self):
        return self.k * 100003 + self.h * 1009 + self.w * 17 + self.B

    @property
    def id(self):
        return f"{self.name}-{self.h}x{self.w}b{self.B}"


def cases(names=None, shapes=None):
    out = []
    for name, k, prefix, ch, st in BLOCKS:
        if names is not None and name not in names:
            continue
        for h, w, B in _SHAPES[ch]:
            if shapes is None or (h, w, B) in shapes:
                out.append(Case(name, k, prefix, ch, st, h, w, B))
    return out


def block(name):
    return next(b for b in BLOCKS if b[0] == name)


@functools.lru_cache(maxsize=None)
def state_dict():
    from vstnet_amd.synth import synthetic_state_dict
    return synthetic_state_dict(1234, 16, 2)


def src_of(case):
    """unit-normal F input of a case (float32; no ReLU-dead or saturating values), one seed per case"""
    g = torch.Generator().manual_seed(case.seed)
    return torch.randn(*case.src_shape, generator=g)


# ------------------------------------------------------------------------------------------- references and models (CPU)
def _double(sd, prefix):
    return {k: v.double() for k, v in sd.items() if k.startswith(prefix)}


def F64(x2, sd, prefix, stride):
    """cpu_ref.residual_F on fp64 copies of the input and of the block's parameters"""
    with torch.no_grad():
        return cpu_ref.residual_F(x2.double(), _double(sd, prefix), prefix, stride)


def reference_weights(sd, prefix, mode):
    """the state dict whose F64 a mode is compared with: fp16-rounded weights for the fp16 modes, the exact ones otherwise"""
    return emul.rounded_weights(sd, prefix) if mode in ("f16x2", "f16x2h") else sd


def e32(x2, sd, prefix, stride):
    """(rel-L2, max-rel) of the oracle's float32 residual_F against F64"""
    with torch.no_grad():
        return rel_err(cpu_ref.residual_F(x2.float(), sd, prefix, stride), F64(x2, sd, prefix, stride))


def _conv_chain32(x, w, b, stride):
    """One conv as conv_fp32_kernel sums it (vstnet_amd/csrc/conv.hip, `float acc = a.bias[co]; for (tap) ... for (ci) acc =
    fmaf(p[ci], w[ci * COUT], acc)`): ONE float32 accumulator per output, started at the bias, the 9 CIN products added one after
    the other, taps outer, input channels inner.  Each step is done in fp64 (the product of two float32 is exact there) and
    rounded to float32, which is fmaf up to a double rounding."""
    B, cin = x.shape[:2]
    cout = w.shape[0]
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), mode="reflect"), 3, stride=stride)               # [B, cin * 9, L], channel-major
    L = cols.shape[-1]
    cols = cols.view(B, cin, 9, L).permute(2, 1, 0, 3).reshape(9 * cin, B * L).double()     # [tap * cin + ci, pixel]
    wk = w.reshape(cout, cin, 9).permute(2, 1, 0).reshape(9 * cin, cout).double()
    acc = b.float().double().expand(B * L, cout).contiguous()
    for k in range(9 * cin):
        acc = torch.addcmul(acc, cols[k][:, None], wk[k][None, :]).float().double()
    ho = (x.shape[2] - 1) // stride + 1
    return acc.float().view(B, ho, L // ho, cout).permute(0, 3, 1, 2).contiguous()


def chain32_F(x2, sd, prefix, stride):
    """the model of VST_PREC_FP32: residual_F in float32 with every conv summed as one serial chain (_conv_chain32)"""
    with torch.no_grad():
        h = x2.float()
        for i in (1, 4, 7):
            h = _conv_chain32(h, sd[prefix + f"conv.{i}.weight"], sd[prefix + f"conv.{i}.bias"], stride if i == 1 else 1)
            if i != 7:
                h = F.relu(h)
    return h


def model_error(x2, sd, prefix, stride, channel, mode):
    """(rel-L2, max-rel) of the mode's model against the mode's F64.  The MFMA modes: emul.residual_F evaluated in fp64, the
    operand roundings alone.  fp32: chain32_F, the kernel's own summation order - see MODEL CORRECTION below."""
    if mode == "fp32":
        return rel_err(chain32_F(x2, sd, prefix, stride), F64(x2, sd, prefix, stride))
    with torch.no_grad():
        m = emul.residual_F(x2.double(), _double(sd, prefix), prefix, stride, mode, channel)
    return rel_err(m, F64(x2, reference_weights(sd, prefix, mode), prefix, stride))


def _conv(x, w, b, stride=1):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b, stride=stride)


def dropped_term_model(x2, sd, prefix, stride, conv):
    """A fault the bf16x3 bound must reject: emul's bf16x3 model in fp64 with w_lo zeroed on tap row 0 of the first min(32, CIN)
    input channels of conv.`conv` - the w_lo x_hi MFMAs of one tap row of one 32-channel chunk lost."""
    d = _double(sd, prefix)
    q = emul.bf16x2
    h = x2.double()
    with torch.no_grad():
        for i in (1, 4, 7):
            w = d[prefix + f"conv.{i}.weight"]
            wq = q(w)
            if i == conv:
                n = min(32, w.shape[1])
                wq = wq.clone()
                wq[:, :n, 0, :] = w[:, :n, 0, :].bfloat16().double()          # w_hi alone
            h = _conv(q(h), wq, d[prefix + f"conv.{i}.bias"], stride if i == 1 else 1)
            if i != 7:
                h = F.relu(h)
    return h


def dropped_xlo_model(x2, sd, prefix, stride):
    """A fault the f16x2 bound must reject: emul's f16x2 model in fp64 with conv.1 reading x_hi alone"""
    d = _double(sd, prefix)
    w1, w4, w7 = (emul.f16(d[prefix + f"conv.{i}.weight"]) for i in (1, 4, 7))
    b1, b4, b7 = (d[prefix + f"conv.{i}.bias"] for i in (1, 4, 7))
    with torch.no_grad():
        h = F.relu(_conv(emul.f16(x2.double()), w1, b1, stride))
        h = F.relu(_conv(emul.f16x2(h), w4, b4))
        return _conv(emul.f16x2(h), w7, b7)


@dataclass(frozen=True)
class Priced:
    ref: torch.Tensor          # F64 of the mode's reference weights
    model: tuple               # (rel-L2, max-rel) of the mode's model
    e32: tuple
    bound: tuple               # 2 x (model + e32), per figure

    def ratios(self, got):
        """(rel-L2, max-rel) of `got` against the reference, each divided by model_error + e32: the bound is 2"""
        l2, mx = rel_err(got, self.ref)
        return l2 / (self.model[0] + self.e32[0]), mx / (self.model[1] + self.e32[1]), l2, mx


def price(x2, sd, prefix, stride, channel, mode, e=None):
    """reference and bound of one mode on any input (e: e32 of that input, where the caller has it already)"""
    m = model_error(x2, sd, prefix, stride, channel, mode)
    e = e32(x2, sd, prefix, stride) if e is None else e
    return Priced(F64(x2, reference_weights(sd, prefix, mode), prefix, stride), m, e, (2 * (m[0] + e[0]), 2 * (m[1] + e[1])))


@functools.lru_cache(maxsize=None)
def case_src(case):
    return src_of(case)


@functools.lru_cache(maxsize=None)
def _case_e32(case):
    return e32(case_src(case), state_dict(), case.prefix, case.stride)


@functools.lru_cache(maxsize=None)
def priced_case(case, mode):
    """reference and bound of one case of the table in one mode, computed once and shared"""
    return price(case_src(case), state_dict(), case.prefix, case.stride, case.channel, mode, _case_e32(case))


# ------------------------------------------------------------------------------------------- the dst = 0 runner (GPU)
@dataclass
class Ran:
    fwd: torch.Tensor          # +F(src) as [B, channel, h, w], float32, on the CPU
    inv: torch.Tensor          # what direction -1 left in a zero dst: -F(src)
    spare_intact: bool         # the image after the batch in dst still holds the sentinel, both directions
    src_intact: bool           # src is bitwise what it was, both directions
    again_same: bool           # a second call into the same buffers (dst zeroed again, tmp as the first call left it): same bits


def run_F(L, weights, k, channel, stride, precision, x2):
    """vst_block_apply on dst = 0 in both directions.  x2: F's input as an NCHW view (finer level for stride 2, as run_block of
    tests/test_gpu_parity.py takes it).  dst is a zero state of the same frame; read back at the block's own level it is what
    squeezing the finer view of a stride-2 block's dst gives (the same memory).  dst has one image more than the call is told of,
    filled with a sentinel."""
    B = x2.shape[0]
    src = nchw_to_zc(x2.float()).cuda()
    Hq, Wq = src.shape[1], src.shape[2]
    H, W = 4 * Hq, 4 * Wq
    src0 = src.clone()
    from vstnet_amd import _lib
    tmp = torch.zeros(L.vst_block_tmp_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    res, spare_ok, src_ok, again = {}, True, True, True
    for direction in (+1, -1):
        dst = torch.zeros(B + 1, Hq, Wq, 256, device="cuda")
        dst[B] = SENTINEL
        for rep in range(2):
            dst[:B] = 0
            rc = L.vst_block_apply(C.byref(weights.blocks[k]), channel, stride, direction, precision, ptr(dst), ptr(src), ptr(tmp),
                                   B, H, W, stream())
            _lib.check(rc, "vst_block_apply")
            out = dst.cpu()
            spare_ok &= bool((out[B] == SENTINEL).all())
            src_ok &= torch.equal(src, src0)
            if rep == 0:
                res[direction] = out[:B]
            else:
                again &= torch.equal(out[:B].view(torch.int32), res[direction].view(torch.int32))
    return Ran(zc_to_nchw(res[+1], channel), zc_to_nchw(res[-1], channel), spare_ok, src_ok, again)


def diluted(got, ref, x1):
    """the figure the golden block test takes: the error of F normalised by the block's output x1 + F"""
    return rel_err(x1.double() + got.double(), x1.double() + ref.double())
