"""CPU: the per-block bound of tests/block_ref.py rejects what it is meant to catch - shown on models of faulty kernels, without
a GPU and without mutating a kernel - and the golden block test's way of normalising (by the block's output x1 + F) does not.

Figures on the synthetic checkpoint, unit-normal states, 20 x 36 with B = 3 (rel-L2 / max-rel):

  fault                                         of F                   bound (2 x (model + e32))   of x1 + F              old bound
  stack.25. conv.1, w_lo lost on a tap row      3.36e-04 / 3.79e-04    1.21e-05 / 1.23e-05         3.38e-05 / 4.19e-05    2e-5
  stack.3.  conv.1, the same                    1.27e-03 / 1.87e-03    1.44e-05 / 1.57e-05         9.24e-05 / 1.55e-04    2e-5
  stack.13. conv.7, the same                    1.04e-03 / 1.14e-03    1.29e-05 / 1.22e-05         1.11e-04 / 1.32e-04    2e-5
  stack.25. conv.1 reads x_hi alone (f16x2)     1.94e-04 / 2.10e-04    7.88e-07 / 8.79e-07         1.95e-05 / 2.33e-05    3e-4
  stack.3.  the same                            2.63e-04 / 2.98e-04    8.68e-07 / 1.18e-06         1.92e-05 / 2.48e-05    3e-4
  stack.13. the same                            2.04e-04 / 1.91e-04    8.24e-07 / 9.06e-07         2.17e-05 / 2.20e-05    3e-4

Every fault is 25 to 300 times over the new bound.  Normalised by x1 + F each shrinks about tenfold (F has rms ~ 0.1 beside a
unit-normal x1).  The three fp16 faults then sit more than ten times UNDER the old 3e-4: a kernel that never reads x_lo passes
the golden block test.  A whole tap row of w_lo lost in bf16x3 stays over the old 2e-5 on these states (by 1.7 x for the
256-channel block), a third of that row (one 32-deep k step of stack.25. conv.1: 1.9e-4 of F, 1.9e-5 / 2.3e-5 of x1 + F) sits on it.
"""
import pytest
import torch

from tests import block_ref as br
from tests import emul
from tests.zc import rel_err

OLD_BOUND = {"bf16x3": 2e-5, "f16x2": 3e-4}            # test_block_golden's parametrisation (tests/test_gpu_parity.py)
SHAPE = [(20, 36, 3)]
DROPPED_TERM = [("c256s1", 1), ("c16s1", 1), ("c64s1", 7)]


def _case(name):
    (c,) = br.cases([name], SHAPE)
    return c


def _x1(ref):
    return torch.randn(ref.shape, generator=torch.Generator().manual_seed(7))


@pytest.mark.parametrize("name,conv", DROPPED_TERM)
def test_bf16x3_bound_rejects_a_lost_w_lo_term(name, conv):
    c = _case(name)
    p = br.priced_case(c, "bf16x3")
    faulty = br.dropped_term_model(br.case_src(c), br.state_dict(), c.prefix, c.stride, conv)
    l2, mx = rel_err(faulty, p.ref)
    print(f"{name} conv.{conv}: w_lo lost on a tap row: {l2:.3e} / {mx:.3e} of F, bound {p.bound[0]:.3e} / {p.bound[1]:.3e}")
    assert l2 >= 5 * p.bound[0] and mx >= 5 * p.bound[1]
    # the same output the old way: about ten times smaller, since F is a tenth of x1 + F
    dl2, dmx = br.diluted(faulty, p.ref, _x1(p.ref))
    print(f"    of x1 + F: {dl2:.3e} / {dmx:.3e} (old bound {OLD_BOUND['bf16x3']:g})")
    assert l2 >= 8 * dl2


@pytest.mark.parametrize("name", ["c256s1", "c16s1", "c64s1"])
def test_f16x2_bound_rejects_a_lost_x_lo_and_the_old_bound_does_not(name):
    c = _case(name)
    p = br.priced_case(c, "f16x2")
    faulty = br.dropped_xlo_model(br.case_src(c), br.state_dict(), c.prefix, c.stride)
    l2, mx = rel_err(faulty, p.ref)
    print(f"{name}: conv.1 reads x_hi alone: {l2:.3e} / {mx:.3e} of F, bound {p.bound[0]:.3e} / {p.bound[1]:.3e}")
    assert l2 >= 5 * p.bound[0] and mx >= 5 * p.bound[1]
    # ... and the old test's figure for the same faulty output, against the exact weights as that test has it, is inside its bound
    exact = br.F64(br.case_src(c), br.state_dict(), c.prefix, c.stride)
    dl2, dmx = br.diluted(faulty, exact, _x1(exact))
    print(f"    of x1 + F: {dl2:.3e} / {dmx:.3e} (old bound {OLD_BOUND['f16x2']:g})")
    assert dl2 <= OLD_BOUND["f16x2"] and dmx <= OLD_BOUND["f16x2"]


def test_the_models_pass_their_own_bounds():
    """the sound model of each mode is inside 2 x (model + e32) by construction; a bound that its own model missed would be a typo"""
    for c in br.cases(None, SHAPE):
        for mode in ("bf16x3", "f16x2", "f16x2h"):
            p = br.priced_case(c, mode)
            with torch.no_grad():
                sd64 = {k: v.double() for k, v in br.state_dict().items() if k.startswith(c.prefix)}
                m = emul.residual_F(br.case_src(c).double(), sd64, c.prefix, c.stride, mode, c.channel)
            r = p.ratios(m)
            assert r[0] <= 1.0 and r[1] <= 1.0, (c.id, mode, r)


def test_case_table():
    """every block kind at every shape class; frames legal for the C ABI (multiples of 4, >= 8)"""
    cs = br.cases()
    assert {c.name for c in cs} == {b[0] for b in br.BLOCKS} and len(cs) == 29
    for c in cs:
        H, W = c.frame
        assert H % 4 == 0 and W % 4 == 0 and H >= 8 and W >= 8, c.id
        assert (20, 36, 3) in [(k.h, k.w, k.B) for k in cs if k.name == c.name]
    assert len({c.seed for c in cs}) == len(cs)


def test_emul_float32_results_unchanged():
    """the dtype-preserving helpers on float32 input == the `.half().float()` formulas they replaced, bit for bit"""
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-4, torch.randn(4096, generator=g) * 3e4,
                   torch.tensor([0.0, -0.0, 65504.0, -65504.0, 65520.0, 1e6, -1e6, 2.0 ** -24, 2.0 ** -25, 6e-8, 1e-30, 3.4e38])])
    bits = lambda t: t.view(torch.int32)
    old_f16 = x.clamp(-65504.0, 65504.0).half().float()
    old_f16x2 = old_f16 + (x - old_f16).half().float()
    hb = x.bfloat16().float()
    old_bf16x2 = hb + (x - hb).bfloat16().float()
    for new, old in ((emul.f16(x), old_f16), (emul.f16x2(x), old_f16x2), (emul.bf16x2(x), old_bf16x2)):
        assert new.dtype == torch.float32 and torch.equal(bits(new), bits(old))
    # fp64 in, fp64 out, rounded through the narrow type once
    xd = x.double() * (1 + 2.0 ** -30)
    for f in (emul.f16, emul.f16x2, emul.bf16x2):
        assert f(xd).dtype == torch.float64
    assert torch.equal(emul.f16(xd), xd.clamp(-65504.0, 65504.0).half().double())
    # and the chain: residual_F on float32 input is what it was; on fp64 input it runs (it raised on the bias dtype before)
    sd, c = br.state_dict(), _case("c64s1")
    x2 = br.case_src(c)[:1]
    with torch.no_grad():
        for mode in ("bf16x3", "f16x2", "f16x2h"):
            a = emul.residual_F(x2, sd, c.prefix, 1, mode, 64)
            assert a.dtype == torch.float32
            b = emul.residual_F(x2.double(), {k: v.double() for k, v in sd.items()}, c.prefix, 1, mode, 64)
            # (close, not equal: a float32 rounding of h1 / h2 can flip the narrow rounding that follows, one unit of the mode)
            assert b.dtype == torch.float64 and rel_err(a, b)[1] < {"bf16x3": 2.0 ** -16, "f16x2": 2.0 ** -20, "f16x2h": 2.0 ** -10}[mode]


def test_rounded_weights():
    sd = br.state_dict()
    r = emul.rounded_weights(sd, "stack.13.")
    assert sorted(r) == sorted(k for k in sd if k.startswith("stack.13."))
    for k, v in r.items():
        if k.endswith("bias"):
            assert v is sd[k]
        else:
            assert torch.equal(v, sd[k].half().float()) and not torch.equal(v, sd[k])
