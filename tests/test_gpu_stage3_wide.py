"""VST_OPT_STAGE3_WIDE (vstnet.h): the pipelined stage-3 convs as 4 waves on the 16 x 16 tile (one wave per SIMD, 4 tile rows
each) give the same bits as the 8-wave form - same LDS images, fragments and MFMA order per accumulator."""
import pytest
import torch

from vstnet_amd import _lib
from vstnet_amd.synth import synthetic_frames, synthetic_state_dict

SHAPES = [("photo", 1, (1024, 1024)), ("photo", 1, (200, 280)), ("photo", 1, (72, 40)), ("art", 3, (136, 104)),
          ("photo", 2, (1080, 360))]


def make_net(mode, precision, seed=1234):
    from models.RevResNet import RevResNet
    hd, sp = (16, 2) if mode == "photo" else (64, 1)
    net = RevResNet(hidden_dim=hd, sp_steps=sp, precision=precision)
    net.load_state_dict(synthetic_state_dict(seed, hd, sp))
    return net.to("cuda").eval()


def _run_both(mode, precision, batch, shape):
    from models.cWCT import cWCT
    net = make_net(mode, precision)
    cw = cWCT(precision=precision)
    h, w = shape
    xc, xs = synthetic_frames(batch, h, w, seed=0).cuda(), synthetic_frames(batch, h, w, seed=1).cuda()
    res = []
    before_wide, before_lean = _lib.get_option(_lib.OPT_STAGE3_WIDE), _lib.get_option(_lib.OPT_STAGE3_LEAN)
    try:
        _lib.set_option(_lib.OPT_STAGE3_LEAN, 0)
        with torch.no_grad():
            for wide in (0, 1):
                _lib.set_option(_lib.OPT_STAGE3_WIDE, wide)
                assert _lib.get_option(_lib.OPT_STAGE3_WIDE) == wide
                zc = net(xc)
                sty = net(cw.transfer(zc, net(xs)), forward=False)
                res.append((torch.as_tensor(zc).float().clone(), sty.clone()))
    finally:
        _lib.set_option(_lib.OPT_STAGE3_WIDE, before_wide)
        _lib.set_option(_lib.OPT_STAGE3_LEAN, before_lean)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("mode,batch,shape", SHAPES)
def test_stage3_wide_option_is_bit_identical(mode, batch, shape):
    """Full size, ragged tiles, a frame smaller than a tile, an artistic batch, a tall batch whose quarter-resolution height (270)
    is not a multiple of 16."""
    res = _run_both(mode, "bf16x3", batch, shape)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2h"])
def test_stage3_wide_option_is_bit_identical_per_precision(precision):
    """Every precision that reaches the pipelined kernel (block 20's conv.4 / conv.7 included) at a ragged size."""
    res = _run_both("photo", precision, 1, (264, 200))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.gpu
def test_stage3_lean_over_wide_is_bit_identical():
    """VST_OPT_STAGE3_LEAN takes precedence over VST_OPT_STAGE3_WIDE and gives the same bits."""
    assert _lib.get_option(_lib.OPT_STAGE3_WIDE) in (0, 1)
    before = _lib.get_option(_lib.OPT_STAGE3_LEAN)
    try:
        res = []
        net = make_net("photo", "bf16x3")
        x = synthetic_frames(1, 200, 280, seed=3).cuda()
        with torch.no_grad():
            for lean in (0, 1):
                _lib.set_option(_lib.OPT_STAGE3_LEAN, lean)
                res.append(torch.as_tensor(net(x)).float().clone())
    finally:
        _lib.set_option(_lib.OPT_STAGE3_LEAN, before)
    assert torch.equal(res[0], res[1])
