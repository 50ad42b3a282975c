"""VST_OPT_STAGE1_FOLD and VST_OPT_OUT_RGB (vstnet.h).

Fold: conv.1 of the 16-channel blocks (bf16x3) with the horizontal tap in the weight operand's rows and a shift-add of the three
partial sums afterwards - the same products in another order, so it is held to the per-block bf16x3 bound of
tests/test_gpu_parity.py (taken from that file's parametrisation) against an fp64 CPU evaluation of the same fp32 inputs, and
against the unfolded form of the same build, border pixels on their own (a wrong shift shows there first).

RGB: the last block of an inverse pass writes the image from its epilogue instead of the state + unpack launch: bit-identical.
"""
import pytest
import torch

from oracle import cpu_ref
from tests import test_gpu_parity as parity
from tests.zc import rel_err
from vstnet_amd import _lib
from vstnet_amd.synth import synthetic_frames

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _block_tol():
    """the (bf16x3, tol) entry of test_block_golden's parametrisation"""
    for m in parity.test_block_golden.pytestmark:
        if m.name == "parametrize" and m.args[0] == "precision,tol":
            return dict(m.args[1])[_lib.PREC_BF16X3]
    raise AssertionError("tests/test_gpu_parity.py::test_block_golden no longer carries a bf16x3 bound")


BLOCK_TOL = _block_tol()
K, PREFIX = 3, "stack.3."                       # the 16-channel block the golden file covers


class _option:
    def __init__(self, opt, value):
        self.opt, self.value = opt, value

    def __enter__(self):
        self.before = _lib.get_option(self.opt)
        _lib.set_option(self.opt, self.value)
        assert _lib.get_option(self.opt) == self.value

    def __exit__(self, *exc):
        _lib.set_option(self.opt, self.before)


def _inputs(shape_hw, seed):
    g = torch.Generator().manual_seed(seed)
    h, w = shape_hw
    return torch.randn(1, 16, h, w, generator=g), torch.randn(1, 16, h, w, generator=g)


def _both_directions(L, net, x1, x2, H, W):
    """(y1 of the forward block, x1 of the inverse block) on the GPU in bf16x3"""
    y1 = parity.run_block(L, net, K, 16, 1, +1, _lib.PREC_BF16X3, x1, x2, H, W)
    x1r = parity.run_block(L, net, K, 16, 1, -1, _lib.PREC_BF16X3, x1, x2, H, W)
    return y1, x1r


def _ref64(sd, x1, x2):
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(PREFIX)}
    f = cpu_ref.residual_F(x2.double(), sd64, PREFIX, 1)
    return x1.double() + f, x1.double() - f


def _border(t):
    m = torch.zeros(t.shape[-2:], dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return t[..., m]


# 64 x 64: tile-interior; 24 x 40: the golden's ragged shape; 40 x 52: a width that is not a multiple of 16 beyond the first tile;
# 20 x 16 / 16 x 36: a last tile row of 4 rows, a last tile column of 4 columns
SHAPES = [(64, 64), (24, 40), (40, 52), (20, 16), (16, 36)]


@pytest.mark.parametrize("shape", SHAPES)
def test_folded_conv1_against_fp64(shape):
    L = _lib.lib()
    net, sd, _ = parity.make_net("photo")
    x1, x2 = _inputs(shape, 11)
    ref = _ref64(sd, x1, x2)
    with _option(_lib.OPT_STAGE1_FOLD, 1):
        got = _both_directions(L, net, x1, x2, *shape)
    for what, g, r in zip(("forward y1", "inverse x1"), got, ref):
        l2, mx = rel_err(g, r)
        assert l2 <= BLOCK_TOL and mx <= BLOCK_TOL, f"folded {what} {shape}: rel-L2 {l2:.3e}, max-rel {mx:.3e} (bound {BLOCK_TOL:g})"


def test_folded_block_golden(golden):
    """the reference's own block outputs (tests/golden/blocks.npz), as test_block_golden, with the option forced on"""
    L = _lib.lib()
    g = golden("blocks")
    net, _, _ = parity.make_net("photo")
    x1, x2 = T(g["c16s1_x1"]), T(g["c16s1_x2"])
    H, W = x1.shape[2], x1.shape[3]
    with _option(_lib.OPT_STAGE1_FOLD, 1):
        y1 = parity.run_block(L, net, K, 16, 1, +1, _lib.PREC_BF16X3, x1, x2, H, W)
        x1r = parity.run_block(L, net, K, 16, 1, -1, _lib.PREC_BF16X3, T(g["c16s1_out_y1"]), T(g["c16s1_out_x2"]), H, W)
    for what, got, ref in (("forward y1", y1, T(g["c16s1_out_y1"])), ("inverse x1", x1r, T(g["c16s1_inv_x1"]))):
        l2, mx = rel_err(got, ref)
        assert l2 <= BLOCK_TOL and mx <= BLOCK_TOL, f"folded golden {what}: rel-L2 {l2:.3e}, max-rel {mx:.3e} (bound {BLOCK_TOL:g})"


@pytest.mark.parametrize("shape", SHAPES)
def test_folded_against_unfolded(shape):
    L = _lib.lib()
    net, _, _ = parity.make_net("photo")
    x1, x2 = _inputs(shape, 12)
    res = []
    for fold in (0, 1):
        with _option(_lib.OPT_STAGE1_FOLD, fold):
            res.append(_both_directions(L, net, x1, x2, *shape))
    for what, a, b in zip(("forward y1", "inverse x1"), res[0], res[1]):
        l2, mx = rel_err(b, a)
        scale = float(a.abs().max())
        bd = float((_border(a.double()) - _border(b.double())).abs().max()) / scale
        msg = f"folded vs unfolded {what} {shape}: rel-L2 {l2:.3e}, max-rel {mx:.3e}, border max-rel {bd:.3e} (bound {BLOCK_TOL:g})"
        assert l2 <= BLOCK_TOL and mx <= BLOCK_TOL and bd <= BLOCK_TOL, msg


def test_fold_option_leaves_other_modes_alone():
    """fp32 and the fp16 modes never take the folded kernel: the option changes no bit there"""
    L = _lib.lib()
    net, _, _ = parity.make_net("photo")
    x1, x2 = _inputs((24, 40), 13)
    for prec in (_lib.PREC_FP32, _lib.PREC_F16X2, _lib.PREC_F16X2H):
        res = []
        for fold in (0, 1):
            with _option(_lib.OPT_STAGE1_FOLD, fold):
                res.append(parity.run_block(L, net, K, 16, 1, +1, prec, x1, x2, 24, 40))
        assert torch.equal(res[0], res[1]), prec


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2", "f16x2h"])
@pytest.mark.parametrize("batch,shape", [(1, (1024, 1024)), (1, (24, 40)), (2, (24, 40)), (1, (200, 280))])
def test_out_rgb_is_bit_identical(precision, batch, shape):
    """decode with the image written by the last block's epilogue == decode through the state and the unpack launch: float and
    uint8 edge, packed code (one image) and dense code (a batch of small images)"""
    if precision != "bf16x3" and shape == (1024, 1024):
        shape = (264, 200)                          # (the bench shape in the bench precision; a ragged one in the others)
    net, _, _ = parity.make_net("photo", precision)
    x = synthetic_frames(batch, *shape, seed=5).cuda()
    res = []
    with torch.no_grad():
        z = net(x)
        for rgb in (0, 1):
            with _option(_lib.OPT_OUT_RGB, rgb):
                res.append((net(z, forward=False).clone(), net.inverse_u8(z).clone()))
    assert res[0][0].shape == x.shape and res[0][1].shape == (batch, *shape, 3)
    assert torch.equal(res[0][0], res[1][0]), "float image"
    assert torch.equal(res[0][1], res[1][1]), "uint8 frames"
    assert float((res[1][0] - x).abs().max()) < 1e-2       # and it is the image


def test_out_rgb_dense_code_and_pending_transfer():
    """a plain [B,32,H,W] tensor code (vst_revnet_inverse) and a packed code with a pending cWCT map (vst_revnet_decode + affines)"""
    from models.cWCT import cWCT
    net, _, _ = parity.make_net("photo", "bf16x3")
    cw = cWCT(precision="bf16x3")
    xc, xs = synthetic_frames(1, 72, 104, seed=0).cuda(), synthetic_frames(1, 72, 104, seed=1).cuda()
    res = []
    with torch.no_grad():
        zc, zs = net(xc), net(xs)
        dense = torch.as_tensor(zc).float().clone()
        zcs = cw.transfer(zc, zs)
        for rgb in (0, 1):
            with _option(_lib.OPT_OUT_RGB, rgb):
                res.append((net(dense, forward=False).clone(), net.inverse_u8(dense).clone(), net(zcs, forward=False).clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_out_rgb_profile_table_has_no_unpack():
    """the launch is reported under the pair kernel's id; no unpack entry for a decode"""
    net, _, _ = parity.make_net("photo", "bf16x3")
    x = synthetic_frames(1, 64, 96, seed=7).cuda()
    UNPACK = 2                                   # vstnet.h VST_KERNEL_UNPACK
    with torch.no_grad():
        z = net(x)
        torch.cuda.synchronize()
        tables = []
        for rgb in (0, 1):
            with _option(_lib.OPT_OUT_RGB, rgb):
                t = _lib.profile_table(lambda: net(z, forward=False))
                tables.append({k: v[1] for k, v in t.items()})
    assert tables[0].get(UNPACK) == 1 and UNPACK not in tables[1], tables
    pair = _lib.kernel_id(4, 16, 1)
    assert tables[0][pair] == tables[1][pair] == 10
    assert {k: v for k, v in tables[0].items() if k != UNPACK} == tables[1]
