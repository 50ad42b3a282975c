"""CPU: the one-live-block-per-pass method of tests/pass_ref.py is what it says - against the oracle's whole passes - and its bound
rejects the faults it is meant to catch, shown on the oracle's result without a GPU and without mutating a kernel.

Figures (synthetic checkpoint, unit-normal states; error / priced sum, the bound is 2; rel-L2 / max-rel; bf16x3, f16x2, f16x2h):

  fault                                                     case             ratio
  (a) the dst half of one chain position through hi only:
      on the F half                                         fwd25 80x144     - , 367 / 500, 0.6 / 0.7 (*)
      on the half that passes through                       fwd25 80x144     959 x the per-element allowance (bound 1), both fp16 modes
      what a whole-network comparison sees of the latter    1.47e-4 rel-L2 of a state of x's size: inside NET_TOL = 2e-4
  (b) result = x + F (old values taken from the src buffer) fwd25 80x144     1.6e6, 1.7e7, 2.9e4
  (c) one 16 x 16 tile of F from a zero src                 fwd25 80x144     5.1e4 / 1.5e5, 5.5e5 / 1.8e6, 918 / 2367
  (d) the fold constant with a wrong tap order (+)          fwd0 20x36, x=0  2.1e6, 4.5e5, 4.5e5; with unit-normal x 4.8e5 / 9.2e4, 2.1e5 / 2.8e4
  (e) image channel c taken from channel c + 1, C_out = 5   inv0 20x36       2.1e5, 2.7e6, 4584 / 2751; with unit-normal s0 ten times that

  (*) f16x2h prices F itself at single-fp16 h1 / h2 (3e-4 of F): a 2^-12 rounding of the F half is inside that mode's own error and
      no bound on F can see it there; the same fault on the other half is caught in both modes.
  (+) the taps-major formula of block0_const_kernel applied to the weights in OIHW order.  A transposition of the 3 x 3 taps among
      themselves is not a fault of the fold: F_0(0) sums a constant field over all taps (shown in the same test).

One figure of the issue could not hold as stated: "fewer than 1 % of the oracle's values within delta of an integer" for the uint8
output.  In bf16x3 and f16x2 it does (0.4 % and 0.08 % at most).  In f16x2h delta = 255 x the mode's own bound is 0.07 .. 0.11 of
a byte step, so 13 .. 21 % of all values are that close whatever the seed; the card's test still holds that mode to a step of 1,
only at such values, and to 1 % of the bytes (measured: 0.2 .. 0.4 %).
"""
import pytest
import torch

from oracle import cpu_ref
from tests import block_ref as br
from tests import emul
from tests import pass_ref as pr
from tests.zc import rel_err

NET_TOL = 2e-4                                          # tests/test_gpu_parity.py: the whole-network tolerance of f16x2
MFMA_MODES = ("bf16x3", "f16x2", "f16x2h")


def _x(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).double()


def _sd64(k):
    return {n: v.double() for n, v in pr.live_sd(k).items()}


# ------------------------------------------------------------------------------------------- the construction
@pytest.mark.parametrize("k", range(32))
def test_live_block_against_the_oracles_whole_passes(k):
    """forward_live / inverse_live == cpu_ref.revnet_forward / revnet_inverse of the live state dict, bit for bit; the share of
    outputs that block k changes is 0.5 (forward, odd k), 1.0 (inverse, even k), 0.0 (inverse, odd k)"""
    sd = _sd64(k)
    zero = _sd64(None)
    x = _x((2, 16, 8, 12), 100 + k)
    with torch.no_grad():
        z_full = cpu_ref.revnet_forward(x, sd, pr.SP)
        z_none = cpu_ref.revnet_forward(x, zero, pr.SP)
        z_live, view = pr.forward_live(x, sd, k)
        assert torch.equal(z_live, z_full) and torch.equal(pr.forward_live(x, {}, None)[0], z_none)
        share = float((z_full != z_none).double().mean())
        if k & 1:
            assert share == 0.5, share
            stride, channel = pr.STACK[k]
            F = br.F64(view, pr.live_sd(k), pr.prefix(k), stride)
            got = (z_full - z_none)[z_full != z_none]
            assert tuple(view.shape[1:]) == (channel // stride ** 2, (8 >> pr.level(k)) * stride, (12 >> pr.level(k)) * stride)
            assert torch.equal(got.sort().values, F.flatten().sort().values)       # +F of the full-width view, nothing added
        else:
            assert float((view != 0).double().mean()) == 0.0                       # src = 0: a constant per channel
        s0, s1 = _x((2, 16, 8, 12), 200 + k), _x((2, 16, 8, 12), 300 + k)
        for dst in (torch.zeros_like(s0), s0):
            z = pr.spread(dst, s1)
            i_full = cpu_ref.revnet_inverse(z, sd, pr.SP, 16)
            i_none = cpu_ref.revnet_inverse(z, zero, pr.SP, 16)
            i_live, view = pr.inverse_live(z, sd, k, 16)
            assert torch.equal(i_live, i_full) and torch.equal(i_none, dst)
            share = float((i_full != i_none).double().mean())
            assert share == (0.0 if k & 1 else 1.0), share
            if not k & 1 and dst is not s0:                                       # s0 = 0: -F undiluted
                stride, _ = pr.STACK[k]
                F = br.F64(view, pr.live_sd(k), pr.prefix(k), stride)
                assert torch.equal((i_none - i_full).flatten().sort().values, F.flatten().sort().values)
        for c in (1, 3, 5):
            assert torch.equal(pr.inverse_live(z, sd, k, c)[0], cpu_ref.revnet_inverse(z, sd, pr.SP, c))


def test_case_tables():
    """every chain position once, legal frames, one seed per case"""
    assert sorted({c.k for c in pr.CHAIN if c.direction > 0}) == list(range(21, 32, 2))      # pos 0, 2, .. 10
    assert sorted({c.k for c in pr.CHAIN if c.direction < 0}) == list(range(22, 31, 2))      # pos 9, 7, .. 1
    assert {(c.H, c.W, c.B) for c in pr.CHAIN} == {(80, 144, 3), (128, 64, 1), (8, 72, 2), (72, 8, 2), (68, 132, 1)}
    assert {c.k for c in pr.STATES if c.direction > 0} == {1, 11, 13} and {c.k for c in pr.STATES if c.direction < 0} == {2, 10, 12, 20}
    assert len(pr.STATES) == 14 and len(pr.PLUMBING) == 18
    every = pr.CHAIN + pr.STATES + pr.FOLD + [c for f in pr.IMAGE_FRAMES for c in pr.image_cases(f) + [pr.image_u8_case(f)]]
    for c in every:
        assert c.H % 4 == 0 and c.W % 4 == 0 and c.H >= 8 and c.W >= 8, c.id
        assert c.direction == pr.observable(c.k) or c.fold, c.id
    assert len({c.id for c in every}) == len(every)


def test_magnitudes_of_F():
    """rms about 0.1, max about 0.4 on unit-normal input; F0(0) about +-0.03 per channel and not trivial"""
    p = pr.priced(pr.Case(25, +1, 80, 144, 3), "bf16x3")
    assert 0.05 < float(p.F.pow(2).mean().sqrt()) < 0.2 and 0.2 < float(p.F.abs().max()) < 0.8
    sd = br.state_dict()
    k0 = br.F64(torch.zeros(1, 16, 8, 8), sd, "stack.0.", 1)
    assert float((k0 - k0[:, :, :1, :1]).abs().max()) < 1e-15                      # a constant per channel (fp64 summation order apart)
    k0 = k0[0, :, 0, 0]
    assert 0.005 < float(k0.abs().max()) < 0.1 and int((k0 != 0).sum()) == 16
    assert 0 < int((sd["stack.0.conv.1.bias"] > 0).sum()) < 4                      # some h1 channels alive, some dead


# ------------------------------------------------------------------------------------------- the pricing
@pytest.mark.parametrize("case", [pr.Case(25, +1, 80, 144, 3), pr.Case(30, -1, 8, 72, 2), pr.Case(13, +1, 40, 72, 3),
                                  pr.Case(10, -1, 8, 36, 2), pr.Case(0, +1, 20, 36, 3, "normal", 3), pr.Case(0, -1, 20, 36, 3, "normal", 5),
                                  pr.Case(0, +1, 8, 264, 1, "u8", 3), pr.Case(0, -1, 32, 16, 1, "zero", 1)], ids=lambda c: c.id)
def test_pricing_is_finite_and_not_zero(case):
    for mode in MFMA_MODES + ("fp32",):
        p = pr.priced(case, mode)
        for i in (0, 1):
            assert 1e-8 < p.total(i) < 1e-2 and p.bound[i] == 2 * p.total(i), (case.id, mode, p)
        f16 = mode in pr.F16_MODES
        assert (p.hop[0] > 0) == f16 and (p.add[0] > 0) == (case.dst != "zero" and (case.fold or not f16))
        assert p.exp.mask.any() and torch.isfinite(p.exp.out).all()
        # the oracle's own result is inside its bound, and so is the mode's model moved through one plane hop
        assert p.ratios(p.exp.out)[:2] == (0.0, 0.0)
        if f16 and case.dst == "zero" and not case.fold:
            stride, channel = pr.STACK[case.k]
            sd64 = {n: v.double() for n, v in br.state_dict().items() if n.startswith(pr.prefix(case.k))}
            with torch.no_grad():
                m = emul.residual_F(p.exp.view, sd64, pr.prefix(case.k), stride, mode, channel)
            l2, mx = rel_err(emul.f16x2(m), br.F64(p.exp.view, br.reference_weights(br.state_dict(), pr.prefix(case.k), mode),
                                                  pr.prefix(case.k), stride))
            assert l2 <= p.total(0) and mx <= p.total(1)


def test_the_split_is_idempotent():
    """emul.f16x2(emul.f16x2(x)) == emul.f16x2(x), the same float32 values (bit for bit but for the sign of a zero: a negative x
    under the 2^-25 floor gives -0, whose own split is +0), on values of every magnitude the planes can hold (normal,
    fp16-subnormal lo, below the floor, near the fp16 range's end): a half that the chain re-splits at every other position is
    still the FIRST split of the input, which is what test_gpu_pass_blocks.py asserts of the half that passes through"""
    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.randn(1 << 20, generator=g) * s for s in (1.0, 1e-2, 1e-4, 3e-7, 100.0, 8e3)]
                  + [torch.tensor([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 - 2.0 ** -12])])
    once = emul.f16x2(x)
    twice = emul.f16x2(once)
    assert torch.equal(twice, once)
    differ = twice.view(torch.int32) != once.view(torch.int32)
    assert bool((once[differ] == 0).all()) and bool((x[differ].abs() < 2.0 ** -25).all())
    d = (once.double() - x.double()).abs()
    assert bool((d <= x.double().abs() * 2.0 ** -22 + 2.0 ** -25).all())           # emul.py's stated 22 bits and floor


@pytest.mark.parametrize("frame", pr.IMAGE_FRAMES, ids=lambda f: "%dx%db%d" % f)
def test_u8_case_has_few_values_near_an_integer(frame):
    """fewer than 1 % of the oracle's 255 v lie within delta of an integer (bf16x3, f16x2), and F pushes values past both clamps"""
    case = pr.image_u8_case(frame)
    for mode in MFMA_MODES:
        ref, near, delta = pr.u8_allowance(case, mode)
        share = float(near.double().mean())
        print(f"{case.id} {mode}: delta {delta:.3e}, share within delta of an integer {share:.4%}")
        assert ref.shape == (frame[2], frame[0], frame[1], 3) and ref.dtype == torch.uint8
        if mode == "f16x2h":
            # single-fp16 h1 / h2 price F at 3e-4: delta is 0.07 .. 0.11 of a byte step and a fifth of all values lie that close
            # to an integer whatever the seed (the share is 2 delta of the unclamped values).  Here "only where near" filters
            # little; the card's test still holds this mode to a step of 1 and to 1 % of the bytes.
            assert 0.02 < delta < 0.2 and 0.5 * delta < share < 3 * delta
        else:
            assert 0 < delta < 0.02 and share < 0.01
    v = pr.expected(case).out
    print(f"{case.id}: {int((v < 0).sum())} values under 0, {int((v > 1).sum())} over 1, of {v.numel()}")
    if frame == (20, 36, 3):                             # (max |F| of the three image channels is about 0.25: the small frames may
        assert bool((v < 0).any()) and bool((v > 1).any()) and int((ref == 0).sum()) > 0 and int((ref == 255).sum()) > 0   # miss a clamp)


# ------------------------------------------------------------------------------------------- the faults
CHAIN_CASE = pr.Case(25, +1, 80, 144, 3)


def _report(what, case, mode, p, faulty):
    rl2, rmx, l2, mx = p.ratios(faulty)
    print(f"{what}: {case.id} {mode}: {l2:.3e} / {mx:.3e} of F = {rl2:.1f} / {rmx:.1f} x the priced sum (bound 2)")
    return rl2, rmx


@pytest.mark.parametrize("mode", pr.F16_MODES)
def test_fault_a_dst_half_through_hi_only(mode):
    """old_sp taking only the hi plane in one chain position: whichever half is dst there is rounded to 11 bits"""
    p = pr.priced(CHAIN_CASE, mode)
    exp = p.exp
    on_F = torch.where(exp.mask, emul.f16(exp.out), exp.out)
    rl2, rmx = _report("(a) F half through hi only", CHAIN_CASE, mode, p, on_F)
    if mode == "f16x2":          # (f16x2h prices F itself at single-fp16 h1 / h2, 3e-4: a 2^-12 rounding of F is inside that mode's
        assert rl2 > 2 and rmx > 2   # own error, there the fault shows on the other half only)
    on_x = torch.where(exp.mask, exp.out, emul.f16(exp.out))
    excess = pr.pass_through_excess(on_x, exp, True)
    print(f"(a) pass-through half through hi only: {excess:.1f} x the allowance (bound 1)")
    assert excess > 2 and not pr.pass_through_is_one_split(on_x, exp)
    assert pr.pass_through_excess(emul.f16x2(exp.out), exp, True) <= 1 and pr.pass_through_is_one_split(emul.f16x2(exp.out), exp)
    # what a whole-network comparison sees of it: there both halves of the state carry values of x's size, so the error of one
    # half is measured against sqrt(2) ||x||
    x = exp.base[~exp.mask]
    for what, faulty in (("F half", on_F), ("pass-through half", on_x)):
        net = float((faulty - exp.out).norm() / (2 ** 0.5 * x.norm()))
        print(f"    whole-network view of the {what}: rel-L2 {net:.3e} of a state of x's size (NET_TOL {NET_TOL:g})")
        assert net < NET_TOL                             # ... which is why the whole-network tests cannot see it


@pytest.mark.parametrize("mode", MFMA_MODES)
def test_fault_b_old_values_from_the_src_buffer(mode):
    p = pr.priced(CHAIN_CASE, mode)
    x = pr.inputs(CHAIN_CASE)["x16"].double()
    faulty = p.exp.out + pr.spread(torch.zeros_like(x), x)           # the s1 half gains x: result = x + F
    assert torch.equal(faulty[~p.exp.mask], p.exp.out[~p.exp.mask])
    rl2, rmx = _report("(b) result = x + F", CHAIN_CASE, mode, p, faulty)
    assert rl2 > 2 and rmx > 2


@pytest.mark.parametrize("mode", MFMA_MODES)
def test_fault_c_one_tile_of_F_from_a_zero_src(mode):
    p = pr.priced(CHAIN_CASE, mode)
    x = pr.inputs(CHAIN_CASE)["x16"].double()
    with torch.no_grad():
        of_zero, _ = pr.forward_live(torch.zeros_like(x), pr._live_sd64(CHAIN_CASE.k, mode in pr.F16_MODES), CHAIN_CASE.k)
    tile = torch.zeros_like(p.exp.mask)
    tile[1, :, 0:64, 64:128] = True                                  # level-2 tile (0, 1) of image 1: a 4 x 4 block of z per cell
    faulty = torch.where(tile & p.exp.mask, of_zero, p.exp.out)
    rl2, rmx = _report("(c) one 16 x 16 tile from a zero src", CHAIN_CASE, mode, p, faulty)
    assert rl2 > 2 and rmx > 2


@pytest.mark.parametrize("mode", MFMA_MODES + ("fp32",))
@pytest.mark.parametrize("dst,c", [("zero", 16), ("normal", 3)])
def test_fault_d_fold_constant_with_a_wrong_tap_order(mode, dst, c):
    """block0_const_kernel (vstnet_amd/csrc/layout.hip) sums w2[(tap * 4 + ci) * 4 + co] over the taps-major fp32 section.  The
    fault: that formula applied to the weights in their OIHW order, w2[(co * 4 + ci) * 9 + tap] - taps and channels transposed.
    (A transposition of the 3 x 3 taps among themselves changes nothing here and cannot be caught by any test: F_0(0) is the sum
    over all taps of a constant field.  The second half of this test shows that.)"""
    case = pr.Case(0, +1, 20, 36, 3, dst, c)
    p = pr.priced(case, mode)
    x = pr.inputs(case)["x16"].double()
    sd = dict(pr._live_sd64(0, False))
    w2 = sd["stack.0.conv.4.weight"]                                               # OIHW [4, 4, 3, 3]
    sd["stack.0.conv.4.weight"] = w2.reshape(9, 4, 4).permute(2, 1, 0).reshape(4, 4, 3, 3).contiguous()
    with torch.no_grad():
        faulty, _ = pr.forward_live(x, sd, 0)
    rl2, rmx = _report("(d) fold constant, taps-major formula on OIHW weights", case, mode, p, faulty)
    assert rl2 > 2 and rmx > 2
    sd["stack.0.conv.4.weight"] = w2.transpose(-1, -2).contiguous()
    with torch.no_grad():
        same, _ = pr.forward_live(x, sd, 0)
    assert max(p.ratios(same)[:2]) < 1e-3                                          # (fp64 summation order only)


@pytest.mark.parametrize("mode", MFMA_MODES)
@pytest.mark.parametrize("dst", ["zero", "normal"])
def test_fault_e_image_channel_from_its_neighbour(mode, dst):
    case = pr.Case(0, -1, 20, 36, 3, dst, 5)
    p = pr.priced(case, mode)
    with torch.no_grad():
        all16, _ = pr.inverse_live(pr.inputs(case)["z"].double(), pr._live_sd64(0, mode in pr.F16_MODES), 0, 16)
    rl2, rmx = _report("(e) image channel c from c + 1", case, mode, p, all16[:, 1:6])
    assert rl2 > 2 and rmx > 2
