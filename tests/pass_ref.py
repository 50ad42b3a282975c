"""How the forms of a coupling block that only a whole pass runs are tested (helper, no tests in it): tests/test_gpu_pass_blocks.py
runs them on the card, tests/test_pass_blocks_host.py checks the construction and what the bound rejects on the CPU.

vst_block_apply (tests/block_ref.py) never executes: forward block 0 folded into the pack kernels (block0_const_kernel + addk),
inverse block 0 writing the image from the pair kernel's epilogue (vst_block0_to_image), the chained vst3_block256(pos = 0..10) of
blocks 21..31 in the fp16 modes (state only in two ping-pong plane buffers, old values from planes, fp32 stored by pos >= 9), and
the sub-batch loop of a pass.  The method: ONE LIVE BLOCK PER PASS.  Zero weights and biases make a block the identity (F == 0
exactly, and vst_normalize_block gives a zero row scale 1), so with every tensor of block_ref.state_dict() zeroed but block k's
six a whole pass through the C ABI is pack -> F_k on a known state -> spread, every other launch of the pass still executed:

  forward, C_in = 16   s0 = x, s1 = 0.  Odd k: the s1 half of z is +F_k(x at k's level) with nothing added, the other half x.
                       Even k: src = 0, F a constant per channel; only k = 0, the fold, is of interest (z's s0 half = x + F_0(0)).
  inverse, C_out = 16  z = spread(s0, s1) built on the CPU: image = s0 - F_k(s1) for even k (s0 = 0: -F_k undiluted); odd k is
                       not observable (k = 31 changes no output element).

The expected values are the oracle's: cpu_ref.revnet_forward / revnet_inverse of the live state dict on fp64 copies, with
emul.rounded_weights in the live block for the fp16 modes.  forward_live / inverse_live below are those two functions with the
31 zero blocks not evaluated (block_forward with F == 0 returns (x2, x1), squeezed at stride 2) - 32 times cheaper, and
tests/test_pass_blocks_host.py shows them equal to the oracle's whole passes bit for bit, for every k.  Which outputs F reaches,
and F's input view for the pricing (the finer view for the stride-2 blocks), come out of those runs - the oracle's own split /
squeeze - not out of a table: F's positions are where the live run differs from the run with no live block.

Bound per case and mode, for rel-L2 and max-rel of the F part (got - pass-through at F's positions, normalised by ||F|| / max |F|):

  bound = 2 x (model_error + e32 + hop) [+ add]

  model_error, e32   block_ref.model_error / block_ref.e32 on F's input view, as block_ref.price has them; the factor 2 is its too.
                     The forward fold is priced as block_ref's fp32 mode in every mode (the constant is evaluated in float32 from
                     the fp32 weight sections: _conv_chain32 + e32) against F64 of the exact weights.
  hop                the fp16 modes only, where every result crosses the split planes once: emul.f16x2(r) - r of the oracle's
                     result r at F's positions (r = F where dst = 0), on the CPU.  0 otherwise.
  add                dst != 0 only: the float32 rounding of the result, 2^-24 |r| per element - for the fold (x + F_0(0) is one
                     float32 addition in the pack kernel) in every mode, for inverse block 0 with a non-zero s0 in bf16x3 (in the
                     fp16 modes the plane hop stands for it).  Added once, outside the factor 2.

`ratios` returns error / (model_error + e32 + hop + add / 2): the bound is 2.  None of these figures comes from the kernels.

No model correction was needed: no case landed above 2 ("The forms only a pass runs", has the measured table).
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import torch

from oracle import cpu_ref
from tests import block_ref as br
from tests import emul
from tests.zc import ptr, stream

SP = 2                                                   # photorealistic mode: z = [B, 32, H, W]
STACK = cpu_ref.STACK + [(1, 256), (1, 256)]             # (stride, channel) of the 32 blocks of a pass
F16_MODES = ("f16x2", "f16x2h")
SPARE_U8 = 77


def prefix(k):
    return f"stack.{k}." if k < 30 else f"channel_reduction.block_list.{k - 30}."


def level(k):
    return {16: 0, 64: 1, 256: 2}[STACK[k][1]]


# ------------------------------------------------------------------------------------------- the live-block state dict
@functools.lru_cache(maxsize=None)
def live_sd(k, rounded=False):
    """block_ref.state_dict() with everything zeroed but block k's six tensors (k = None: all zero); rounded: block k's weights
    through emul.rounded_weights, the reference of the fp16 modes"""
    sd = br.state_dict()
    out = {name: torch.zeros_like(v) for name, v in sd.items()}
    if k is not None:
        live = emul.rounded_weights(sd, prefix(k)) if rounded else sd
        names = [n for n in sd if n.startswith(prefix(k))]
        assert len(names) == 6
        for n in names:
            out[n] = live[n].clone()
    return out


@functools.lru_cache(maxsize=None)
def _live_sd64(k, rounded):
    return {n: v.double() for n, v in live_sd(k, rounded).items() if k is not None and n.startswith(prefix(k))}


# ------------------------------------------------------------------------------------------- the oracle, zero blocks skipped
def forward_live(x, sd, k):
    """cpu_ref.revnet_forward(x, sd, SP) for a state dict whose only non-zero block is k (None: no block).  Returns z and the
    tensor block k's F read (its x2, before the squeeze of a stride-2 block)."""
    x = cpu_ref.inj_pad_fwd(x, 32 - x.shape[1])
    x1, x2 = cpu_ref.split(x)
    view = None
    for i, (stride, _) in enumerate(STACK):
        if i == k:
            view = x2
            x1, x2 = cpu_ref.block_forward(x1, x2, sd, prefix(i), stride)
        else:                                            # block_forward with F == 0
            if stride == 2:
                x1, x2 = cpu_ref.squeeze(x1), cpu_ref.squeeze(x2)
            x1, x2 = x2, x1
    z = cpu_ref.merge(x1, x2)
    for _ in range(SP):
        z = cpu_ref.unsqueeze(z)
    return z, view


def inverse_live(z, sd, k, c_out):
    """cpu_ref.revnet_inverse(z, sd, SP, c_out) for such a state dict, and the tensor block k's F read"""
    for _ in range(SP):
        z = cpu_ref.squeeze(z)
    a, b = cpu_ref.split(z)
    view = None
    for i in range(len(STACK) - 1, -1, -1):
        stride = STACK[i][0]
        if i == k:
            view = cpu_ref.unsqueeze(a) if stride == 2 else a
            a, b = cpu_ref.block_inverse(a, b, sd, prefix(i), stride)
        else:                                            # block_inverse with F == 0
            if stride == 2:
                a, b = cpu_ref.unsqueeze(a), cpu_ref.unsqueeze(b)
            a, b = b, a
    return cpu_ref.inj_pad_inv(cpu_ref.merge(a, b), 32 - c_out), view


def spread(s0, s1):
    """z of the two level-0 state halves [B, 16, H, W], by the oracle's squeeze / merge / unsqueeze"""
    for _ in range(SP):
        s0, s1 = cpu_ref.squeeze(s0), cpu_ref.squeeze(s1)
    z = cpu_ref.merge(s0, s1)
    for _ in range(SP):
        z = cpu_ref.unsqueeze(z)
    return z


# ------------------------------------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Case:
    k: int
    direction: int             # +1: forward pass, -1: inverse pass
    H: int                     # the frame
    W: int
    B: int
    dst: str = "zero"          # what F is added to.  Forward k = 0: x itself, "zero" | "normal" | "u8" (uint8 frames through the
                               # frame entry).  Inverse: s0, "zero" | "normal" | "uniform" ([0.2, 0.8], for the uint8 output)
    c: int = 16                # C_in / C_out of the call

    @property
    def seed(self):
        return self.k * 100003 + self.H * 1009 + self.W * 17 + self.B + (7 if self.direction < 0 else 0)

    @property
    def fold(self):
        return self.direction > 0 and self.k == 0

    @property
    def id(self):
        d = "fwd" if self.direction > 0 else "inv"
        extra = ("" if self.dst == "zero" else "-" + self.dst) + ("" if self.c == 16 else f"-c{self.c}")
        return f"{d}{self.k}-{self.H}x{self.W}b{self.B}{extra}"


def observable(k):
    """the direction in which block k's F reaches the output on a full-width src: forward for odd k, inverse for even k"""
    return +1 if k & 1 else -1


def frames(channel, shapes=None):
    """block_ref's shapes of a level (rows x cols where the block's convs write) as frames of a pass"""
    lv = {16: 0, 64: 1, 256: 2}[channel]
    return [(h << lv, w << lv, B) for h, w, B in br._SHAPES[channel] if shapes is None or (h, w, B) in shapes]


SEAM = (20, 36, 3)
THIN = {16: (8, 20, 2), 64: (4, 18, 2), 256: (2, 18, 2)}       # the thinnest shape of each level in block_ref._SHAPES

# 1. every chain position once: forward k = 21, 23, .. 31 are pos 0, 2, .. 10; inverse k = 30, 28, .. 22 are pos 1, 3, .. 9
CHAIN = [Case(k, observable(k), H, W, B) for k in range(21, 32) for H, W, B in frames(256)]
# 2. blocks whose state has to survive the chain (inverse: fp32 state that only the pos-9 / pos-10 stores produced; forward: their
#    results enter the chain through block 20's planes_a and the fp32 old values of pos 0)
STATES_K = (1, 11, 13, 2, 10, 12, 20)
STATES = [Case(k, observable(k), H, W, B) for k in STATES_K
          for H, W, B in frames(STACK[k][1], [SEAM, THIN[STACK[k][1]]])]
# 3. the same live blocks where the pass calls vst_block_apply (bf16x3; fp32 for k = 1 and k = 20): 20 x 36, B = 3 at the block's level
PLUMBING = [Case(k, observable(k), *frames(STACK[k][1], [SEAM])[0]) for k in tuple(range(21, 32)) + STATES_K]
# 4. the forward fold
FOLD_FRAMES = [(8, 8, 1), (20, 36, 3), (8, 264, 1)]            # 8 x 264: a second 64-wide pack column with a ragged end
FOLD = [Case(0, +1, H, W, B, dst, c) for H, W, B in FOLD_FRAMES
        for dst, c in (("zero", 16), ("normal", 16), ("normal", 3), ("u8", 3))]
# 5. inverse block 0 -> image
IMAGE_FRAMES = [(8, 20, 2), (20, 36, 3), (32, 16, 1)]
IMAGE_C = (1, 3, 5, 16)


def image_cases(frame):
    H, W, B = frame
    out = [Case(0, -1, H, W, B, "zero", c) for c in IMAGE_C]
    if frame == (20, 36, 3):
        out.append(Case(0, -1, H, W, B, "normal", 5))          # the one case with a unit-normal s0
    return out


def image_u8_case(frame):
    return Case(0, -1, *frame, "uniform", 3)


# ------------------------------------------------------------------------------------------- inputs and expected values (CPU)
@functools.lru_cache(maxsize=None)
def inputs(case):
    """forward: {"x": what the call is given, "x16": the oracle's float32 input}; inverse: {"s0", "s1", "z"} (float32)"""
    g = torch.Generator().manual_seed(case.seed)
    shape = (case.B, 16, case.H, case.W)
    if case.direction > 0:
        if case.dst == "u8":
            u8 = torch.randint(0, 256, (case.B, case.H, case.W, 3), generator=g, dtype=torch.uint8)
            # (ToTensor's float32 u8 / 255 is the oracle's input, as it is the reference's)
            return {"x": u8, "x16": (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()}
        x = torch.zeros(shape) if case.fold and case.dst == "zero" else torch.randn(*shape, generator=g)
        x = x[:, :case.c].contiguous()
        return {"x": x, "x16": x}
    s1 = torch.randn(*shape, generator=g)
    s0 = {"zero": lambda: torch.zeros(shape), "normal": lambda: torch.randn(*shape, generator=g),
          "uniform": lambda: torch.rand(*shape, generator=g) * 0.6 + 0.2}[case.dst]()
    return {"s0": s0, "s1": s1, "z": spread(s0, s1)}


@dataclass(frozen=True)
class Expected:
    out: torch.Tensor          # the oracle's fp64 output of the live state dict: z, or the image
    base: torch.Tensor         # the same with no live block: what passes through
    mask: torch.Tensor         # where the two differ: F's positions
    view: torch.Tensor         # F's input (fp64 copy of float32 values)


@functools.lru_cache(maxsize=None)
def expected(case, rounded=False):
    inp = inputs(case)
    with torch.no_grad():
        if case.direction > 0:
            out, view = forward_live(inp["x16"].double(), _live_sd64(case.k, rounded), case.k)
            base, _ = forward_live(inp["x16"].double(), {}, None)
        else:
            out, view = inverse_live(inp["z"].double(), _live_sd64(case.k, rounded), case.k, case.c)
            base, _ = inverse_live(inp["z"].double(), {}, None, case.c)
    return Expected(out, base, out != base, view)


def _rel(d, ref):
    return float(d.norm() / (ref.norm() + 1e-30)), float(d.abs().max() / (ref.abs().max() + 1e-30))


@dataclass(frozen=True)
class Priced:
    exp: Expected
    model: tuple               # (rel-L2, max-rel), of F
    e32: tuple
    hop: tuple
    add: tuple

    @property
    def F(self):
        return (self.exp.out - self.exp.base)[self.exp.mask]

    def total(self, i):
        return self.model[i] + self.e32[i] + self.hop[i] + self.add[i] / 2

    @property
    def bound(self):
        """(rel-L2, max-rel) allowed of the F part: 2 x (model + e32 + hop) + add"""
        return 2 * self.total(0), 2 * self.total(1)

    def errors(self, got):
        """(rel-L2, max-rel) of the F part of `got` (a whole output) against the oracle's"""
        m = self.exp.mask
        return _rel(got.double()[m] - self.exp.out[m], self.F)

    def ratios(self, got):
        """the two errors divided by the priced sum (the bound is 2), and the errors themselves"""
        l2, mx = self.errors(got)
        return l2 / self.total(0), mx / self.total(1), l2, mx


def pricing_mode(case, mode):
    return "fp32" if case.fold else mode


@functools.lru_cache(maxsize=None)
def _view_e32(case):
    stride, channel = STACK[case.k]
    return br.e32(expected(case).view.float(), br.state_dict(), prefix(case.k), stride)


@functools.lru_cache(maxsize=None)
def priced(case, mode):
    """expected values and bound of one case in one mode, every figure from the CPU, computed once and shared"""
    stride, channel = STACK[case.k]
    pm = pricing_mode(case, mode)
    exp = expected(case, rounded=pm in F16_MODES)
    view = exp.view.float()
    model = br.model_error(view, br.state_dict(), prefix(case.k), stride, channel, pm)
    r, Fp = exp.out[exp.mask], (exp.out - exp.base)[exp.mask]
    hop = _rel(emul.f16x2(r) - r, Fp) if mode in F16_MODES else (0.0, 0.0)
    rounding = case.dst != "zero" and (case.fold or mode not in F16_MODES)
    add = _rel(r.abs() * 2.0 ** -24, Fp) if rounding else (0.0, 0.0)
    return Priced(exp, model, _view_e32(case), hop, add)


def pass_through_excess(got, exp, f16):
    """Outside F's positions a pass moves values.  bf16x3 / fp32: unchanged (returns whether they are, as 0.0 / inf).  fp16 modes:
    through hi + lo split planes, |got - x| <= 2^-21 |x| + 2^-24 per element - twice the 22 bits and twice the 2^-25 floor that
    tests/emul.py states for the planes; returns the worst |got - x| over that allowance (<= 1 passes)."""
    m = ~exp.mask
    g, x = got.double()[m], exp.base[m]
    if g.numel() == 0:
        return 0.0
    if not f16:
        return 0.0 if torch.equal(g, x) else float("inf")
    return float(((g - x).abs() / (x.abs() * 2.0 ** -21 + 2.0 ** -24)).max())


def pass_through_is_one_split(got, exp):
    """emul.f16x2 is idempotent in value (tests/test_pass_blocks_host.py shows it on 2^22 values of every magnitude), so however
    often the chain re-splits a half it stays the first split of the input: the same float32 values (the sign of a zero apart)"""
    m = ~exp.mask
    return torch.equal(got.float()[m], emul.f16x2(exp.base.float())[m])


# ------------------------------------------------------------------------------------------- uint8 output
def u8_allowance(case, mode):
    """(expected bytes, may_differ mask, delta): a byte may differ from the quantised fp64 value by 1 and only where 255 v lies
    within delta = 255 x the case's absolute bound of an integer"""
    p = priced(case, mode)
    v = p.exp.out
    delta = 255.0 * p.bound[1] * float(p.F.abs().max())
    t = v * 255.0
    near = (t - t.round()).abs() <= delta
    return cpu_ref.to_uint8(v), near.permute(0, 2, 3, 1).contiguous(), delta


# ------------------------------------------------------------------------------------------- the runner (GPU)
_NETS = {}


def live_weights(k):
    """the packed weights of the live state dict of block k (k = "full": the whole synthetic checkpoint), kept with their net"""
    if k not in _NETS:
        from vstnet_amd.revresnet import RevResNet
        net = RevResNet(hidden_dim=16, sp_steps=SP, precision="bf16x3")
        net.load_state_dict(br.state_dict() if k == "full" else live_sd(k))
        net = net.to("cuda").eval()
        _NETS[k] = (net, net._ensure_packed(torch.device("cuda", torch.cuda.current_device())))
    return _NETS[k][1]


@dataclass
class Ran:
    out: torch.Tensor          # z [B, 32, H, W], the image [B, C_out, H, W] (float32) or the frames [B, H, W, 3] (uint8), on the CPU
    spare_intact: bool         # the image after the batch in the output buffer still holds the sentinel
    src_intact: bool           # the input tensor is bitwise what it was
    again_same: bool           # a second pass into the same, NaN-refilled workspace: same bits
    tail_nan: bool             # float image only: channels >= C_out of a 16-channel NaN-filled buffer are still NaN


def _bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def _run_twice(call, out_of, inp, inp0, ws, refill, intact):
    outs, ok = [], True
    for _ in range(2):
        ws.fill_(255)                                    # NaN as fp32 and as fp16: a stale plane buffer or an unwritten state shows
        refill()
        call()
        outs.append(out_of())
        ok &= intact()
    return outs[0], ok, torch.equal(inp, inp0), torch.equal(_bits(outs[0]), _bits(outs[1]))


def forward_pass(L, weights, precision, x):
    """vst_revnet_forward (x float32 [B, C_in, H, W]) or vst_revnet_forward_u8 (x uint8 [B, H, W, 3])"""
    from vstnet_amd import _lib
    u8 = x.dtype == torch.uint8
    B = x.shape[0]
    H, W = (x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3])
    xd = x.contiguous().cuda()
    x0 = xd.clone()
    ws = torch.empty(L.vst_pass_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    z = torch.empty(B + 1, 32, H, W, device="cuda")

    def refill():
        z[:B] = float("nan")
        z[B] = br.SENTINEL

    def call():
        if u8:
            rc = L.vst_revnet_forward_u8(C.byref(weights), ptr(xd), ptr(z), ptr(ws), B, H, W, SP, precision, stream())
        else:
            rc = L.vst_revnet_forward(C.byref(weights), ptr(xd), ptr(z), ptr(ws), B, x.shape[1], H, W, SP, precision, stream())
        _lib.check(rc, "vst_revnet_forward")

    out, spare, src, again = _run_twice(call, lambda: z[:B].cpu(), xd, x0, ws, refill,
                                        lambda: bool((z[B] == br.SENTINEL).all()))
    return Ran(out, spare, src, again, True)


def inverse_pass(L, weights, precision, z, c_out, u8=False):
    """vst_revnet_inverse into a NaN-filled buffer of 16 channels per image, or vst_revnet_inverse_u8; one spare image behind"""
    from vstnet_amd import _lib
    B, _, H, W = z.shape
    zd = z.contiguous().cuda()
    z0 = zd.clone()
    ws = torch.empty(L.vst_pass_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    plane = H * W
    if u8:
        buf = torch.empty(B + 1, H, W, 3, dtype=torch.uint8, device="cuda")

        def refill():
            buf[:B] = 170
            buf[B] = SPARE_U8

        def call():
            _lib.check(L.vst_revnet_inverse_u8(C.byref(weights), ptr(zd), ptr(buf), ptr(ws), B, H, W, SP, precision, stream()),
                       "vst_revnet_inverse_u8")

        out, spare, src, again = _run_twice(call, lambda: buf[:B].cpu(), zd, z0, ws, refill,
                                            lambda: bool((buf[B] == SPARE_U8).all()))
        return Ran(out, spare, src, again, True)
    buf = torch.empty((B + 1) * 16 * plane, device="cuda")
    n_out, n_img = B * c_out * plane, B * 16 * plane
    tail = []

    def refill():
        buf[:n_img] = float("nan")
        buf[n_img:] = br.SENTINEL

    def call():
        _lib.check(L.vst_revnet_inverse(C.byref(weights), ptr(zd), ptr(buf), ptr(ws), B, c_out, H, W, SP, precision, stream()),
                   "vst_revnet_inverse")
        tail.append(bool(torch.isnan(buf[n_out:n_img]).all()))

    out, spare, src, again = _run_twice(call, lambda: buf[:n_out].view(B, c_out, H, W).cpu(), zd, z0, ws, refill,
                                        lambda: bool((buf[n_img:] == br.SENTINEL).all()))
    return Ran(out, spare, src, again, all(tail))


def run_case(L, case, precision, images=None):
    """one case through the pass entry of its direction (images: a slice of the batch, for the B = 1 comparisons)"""
    inp = inputs(case)
    sl = slice(None) if images is None else images
    w = live_weights(case.k)
    if case.direction > 0:
        return forward_pass(L, w, precision, inp["x"][sl])
    return inverse_pass(L, w, precision, inp["z"][sl], case.c, u8=case.dst == "uniform")
