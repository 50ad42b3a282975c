"""The forms of a coupling block that only a whole pass runs, one live block per pass, on F alone, against fp64.

tests/pass_ref.py has the method, the case tables and the bound - 2 x (model_error + e32 + hop) [+ add] for rel-L2 and max-rel of
the F part, every figure of it computed on the CPU - and tests/test_pass_blocks_host.py shows what that bound rejects.  Every test
prints error / priced sum before it asserts (-s): the bound is 2.  DESIGN.md ("The forms only a pass runs") has the measured table.

Every pass runs twice into a workspace refilled with NaN bytes, into an output buffer with a sentinel image behind the batch.
"""
import pytest
import torch

from tests import block_ref as br
from tests import pass_ref as pr
from tests import test_gpu_parity as parity
from tests.test_gpu_block_tiles import _options
from vstnet_amd import _lib

pytestmark = pytest.mark.gpu
PREC = _lib.PRECISIONS
MFMA_MODES = ("bf16x3", "f16x2", "f16x2h")
ids = lambda cs: [c.id for c in cs]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


_RAN = {}


def ran(L, case, mode, rgb=None):
    """one case in one mode on the card, once per module (the property tests read the same run)"""
    key = (case, mode, rgb)
    if key not in _RAN:
        with _options({} if rgb is None else {_lib.OPT_OUT_RGB: rgb}):
            _RAN[key] = pr.run_case(L, case, PREC[mode])
    return _RAN[key]


def check(case, mode, r, tag=""):
    p = pr.priced(case, mode)
    assert tuple(r.out.shape) == tuple(p.exp.out.shape)
    rl2, rmx, l2, mx = p.ratios(r.out)
    f16 = mode in pr.F16_MODES
    through = pr.pass_through_excess(r.out, p.exp, f16)
    print(f"\nRATIO {case.id} {mode}{tag}: rel-L2 {l2:.3e} = {rl2:.2f} x, max-rel {mx:.3e} = {rmx:.2f} x (model {p.model[0]:.2e} / "
          f"{p.model[1]:.2e} + e32 {p.e32[0]:.2e} / {p.e32[1]:.2e} + hop {p.hop[0]:.2e} / {p.hop[1]:.2e} + add/2 {p.add[0] / 2:.2e} / "
          f"{p.add[1] / 2:.2e}); pass-through {through:.3f} x its allowance")
    assert torch.isfinite(r.out).all(), "an output element was not written, or was computed from the NaN workspace"
    assert r.spare_intact, "the image after the batch was written"
    assert r.src_intact, "the input was written"
    assert r.tail_nan, "channels >= C_out were written"
    assert through <= 1.0, f"{case.id} {mode}{tag}: the half that passes through is {through:.2f} x its allowance"
    if f16:          # the split is idempotent (test_pass_blocks_host.py): however often re-split, still the first split of the input
        assert pr.pass_through_is_one_split(r.out, p.exp), "the half that passes through is not emul.f16x2 of the input"
    assert rl2 <= 2.0 and rmx <= 2.0, f"{case.id} {mode}{tag}: {rl2:.2f} / {rmx:.2f} times the priced sum (bound 2)"


# ------------------------------------------------------------------------------------------- 1. chain positions
@pytest.mark.parametrize("mode", pr.F16_MODES)
@pytest.mark.parametrize("case", pr.CHAIN, ids=ids(pr.CHAIN))
def test_chain_position_against_fp64(L, case, mode):
    """blocks 21..31 as vst3_block256(pos = 0..10): forward k = 21 + pos for even pos, inverse k = 31 - pos for odd pos"""
    check(case, mode, ran(L, case, mode))


# ------------------------------------------------------------------------------------------- 2. states survive the chain
@pytest.mark.parametrize("mode", pr.F16_MODES)
@pytest.mark.parametrize("case", pr.STATES, ids=ids(pr.STATES))
def test_states_survive_the_chain(L, case, mode):
    check(case, mode, ran(L, case, mode))


# ------------------------------------------------------------------------------------------- 3. the pass plumbing, bit for bit
PLUMBING = [(c, "bf16x3") for c in pr.PLUMBING] + [(c, "fp32") for c in pr.PLUMBING if c.k in (1, 20)]


@pytest.mark.parametrize("case,mode", PLUMBING, ids=[f"{c.id}-{m}" for c, m in PLUMBING])
def test_pass_calls_the_block_on_the_right_views(L, case, mode):
    """here the pass calls vst_block_apply: its F part is block_ref.run_F of the same src, bit for bit (level views, s[k & 1]
    roles, spread / gather), and inside the bound like any other"""
    r = ran(L, case, mode)
    check(case, mode, r)
    p = pr.priced(case, mode)
    stride, channel = pr.STACK[case.k]
    alone = br.run_F(L, pr.live_weights(case.k), case.k, channel, stride, PREC[mode], p.exp.view.float())
    F = alone.fwd if case.direction > 0 else alone.inv
    # block_ref's result is in F's own layout; the oracle's pass over it says where each element lands in the output
    carrier = pr.inputs(case)
    with torch.no_grad():
        if case.direction > 0:
            live, _ = pr.forward_live(carrier["x16"].double(), pr._live_sd64(case.k, False), case.k)
        else:
            live, _ = pr.inverse_live(carrier["z"].double(), pr._live_sd64(case.k, False), case.k, case.c)
    ref = br.F64(p.exp.view, br.state_dict(), pr.prefix(case.k), stride)
    m = p.exp.mask
    # same multiset in the same order once both are sorted by the fp64 reference they approximate
    order_pass = (live - p.exp.base)[m].argsort()
    order_alone = (ref if case.direction > 0 else -ref).flatten().argsort()
    got = r.out[m][order_pass]
    assert torch.equal(got.view(torch.int32), F.flatten()[order_alone].view(torch.int32))
    assert alone.spare_intact and alone.src_intact


# ------------------------------------------------------------------------------------------- 4. the forward fold
@pytest.mark.parametrize("mode", MFMA_MODES + ("fp32",))
@pytest.mark.parametrize("case", pr.FOLD, ids=ids(pr.FOLD))
def test_forward_fold_against_fp64(L, case, mode):
    """block0_const_kernel + addk of pack_input_kernel / pack_input_u8_kernel (fp32: the literal three convolutions), against
    F64(0) of the exact weights in every mode; with uint8 frames channels 3..15 still carry F_0(0)[c]"""
    r = ran(L, case, mode)
    check(case, mode, r)
    if case.dst == "zero" and mode != "fp32":            # channels 0..15 of the s0 half are the constant itself: 16 values, where
        p = pr.priced(case, mode)                        # convolutions (fp32 mode, the oracle) differ in the last bit along the borders
        assert r.out[p.exp.mask].unique().numel() == 16


# ------------------------------------------------------------------------------------------- 5. inverse block 0 -> image
@pytest.mark.parametrize("rgb", [1, 0])
@pytest.mark.parametrize("mode", MFMA_MODES)
@pytest.mark.parametrize("frame", pr.IMAGE_FRAMES, ids=lambda f: "%dx%db%d" % f)
def test_inverse_block0_to_image_against_fp64(L, frame, mode, rgb):
    """vst_block0_to_image (conv_pair_kernel<.., OUT_RGB>) for C_out = 1, 3, 5, 16, and the state-plus-unpack route beside it"""
    for case in pr.image_cases(frame):
        check(case, mode, ran(L, case, mode, rgb), f" [OUT_RGB={rgb}]")


@pytest.mark.parametrize("rgb", [1, 0])
@pytest.mark.parametrize("mode", MFMA_MODES)
@pytest.mark.parametrize("frame", pr.IMAGE_FRAMES, ids=lambda f: "%dx%db%d" % f)
def test_inverse_block0_to_uint8(L, frame, mode, rgb):
    """a byte may differ from the quantised fp64 value by 1, only where 255 v lies within delta = 255 x the case's absolute bound
    of an integer, and at most 1 % of the bytes may differ"""
    case = pr.image_u8_case(frame)
    r = ran(L, case, mode, rgb)
    ref, near, delta = pr.u8_allowance(case, mode)
    assert r.out.shape == ref.shape and r.out.dtype == torch.uint8
    d = (r.out.int() - ref.int()).abs()
    share = float((d != 0).double().mean())
    print(f"\nU8 {case.id} {mode} [OUT_RGB={rgb}]: {int((d != 0).sum())} of {d.numel()} bytes differ ({share:.3%}), worst step "
          f"{int(d.max())}, delta {delta:.2e}; {int((ref == 0).sum())} at 0, {int((ref == 255).sum())} at 255")
    assert r.spare_intact and r.src_intact
    assert int(d.max()) <= 1 and bool(near[d != 0].all()) and share <= 0.01


# ------------------------------------------------------------------------------------------- 6. properties, 20 x 36 with B = 3
def _seam(c):
    lv = pr.level(c.k)
    return (c.H >> lv, c.W >> lv, c.B) == pr.SEAM


PROPS = ([(c, m, None) for c in pr.CHAIN + pr.STATES if _seam(c) for m in pr.F16_MODES]
         + [(c, "bf16x3", None) for c in pr.PLUMBING]
         + [(c, m, None) for c in pr.FOLD if _seam(c) for m in MFMA_MODES + ("fp32",)]
         + [(c, m, rgb) for c in pr.image_cases(pr.SEAM) + [pr.image_u8_case(pr.SEAM)] for m in MFMA_MODES for rgb in (1, 0)])
PROP_IDS = [f"{c.id}-{m}" + ("" if rgb is None else f"-rgb{rgb}") for c, m, rgb in PROPS]


@pytest.mark.parametrize("case,mode,rgb", PROPS, ids=PROP_IDS)
def test_second_pass_same_bits_and_buffers_intact(L, case, mode, rgb):
    """a second pass into the same NaN-refilled workspace gives the same bits; the spare image and the input are intact"""
    r = ran(L, case, mode, rgb)
    assert r.again_same and r.spare_intact and r.src_intact and r.tail_nan


@pytest.mark.parametrize("case,mode,rgb", PROPS, ids=PROP_IDS)
def test_batch_image_equals_single_image_pass(L, case, mode, rgb):
    whole = ran(L, case, mode, rgb)
    with _options({} if rgb is None else {_lib.OPT_OUT_RGB: rgb}):
        for b in range(case.B):
            one = pr.run_case(L, case, PREC[mode], images=slice(b, b + 1))
            assert torch.equal(pr._bits(one.out), pr._bits(whole.out[b:b + 1])), f"image {b}"


# ------------------------------------------------------------------------------------------- 7. the sub-batch remainder
_FULL = {}


def _full_net(mode):
    if mode not in _FULL:
        _FULL[mode] = parity.make_net("photo", mode)[0]
    net = _FULL[mode]
    return net._ensure_packed(torch.device("cuda", torch.cuda.current_device()))


def _sub_batch_frame(L, B=3):
    """488 x 480 is the smallest-area frame with a sub-batch of 2 out of 3; the export decides, the next shapes up stand by"""
    for H, W in ((488, 480), (488, 484), (492, 484), (496, 496), (512, 512)):
        if 1 < L.vst_pass_sub_batch(B, H, W) < B:
            return H, W
    raise AssertionError("no frame with 1 < vst_pass_sub_batch(3, H, W) < 3")


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2h"])
def test_sub_batch_remainder(L, mode):
    """a pass whose sub-batch loop ends on a remainder (n < nb): every image equals its own B = 1 pass, forward and inverse"""
    B = 3
    H, W = _sub_batch_frame(L, B)
    nb = L.vst_pass_sub_batch(B, H, W)
    assert 1 < nb < B and B % nb != 0
    w = _full_net(mode)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5))
    fwd = pr.forward_pass(L, w, PREC[mode], x)
    assert torch.isfinite(fwd.out).all() and fwd.spare_intact and fwd.src_intact and fwd.again_same
    inv = pr.inverse_pass(L, w, PREC[mode], fwd.out, 3)
    assert torch.isfinite(inv.out).all() and inv.spare_intact and inv.src_intact and inv.again_same and inv.tail_nan
    print(f"\nSUB-BATCH {H}x{W} B={B}: nb = {nb}; round trip max |x' - x| = {float((inv.out - x).abs().max()):.2e}")
    for b in range(B):
        f1 = pr.forward_pass(L, w, PREC[mode], x[b:b + 1])
        assert torch.equal(f1.out.view(torch.int32), fwd.out[b:b + 1].view(torch.int32)), f"forward, image {b}"
        i1 = pr.inverse_pass(L, w, PREC[mode], fwd.out[b:b + 1], 3)
        assert torch.equal(i1.out.view(torch.int32), inv.out[b:b + 1].view(torch.int32)), f"inverse, image {b}"
    assert float((inv.out - x).abs().max()) < 1e-2       # and it is the image
