"""The wide stage-3 convs (conv_pipe_kernel<..., 4, 4>) with their prologue and tail rearranged: loads issued before the address
arithmetic of the parts that follow, no staging in the stages that have nothing left to stage (peeled last loop iteration).
None of it may change a bit or a store.

Single 256-channel blocks through vst_block_apply, wide against the 8-wave form (whose code is untouched), at the shapes where
the changed code can go wrong (frame -> quarter resolution, where the stage-3 convs write):

   64 x  64 -> 16 x 16       one full tile, reflection on all four sides
   72 x  40 -> 18 x 10       narrower than a tile in one axis, ragged in the other: every store is predicated
  136 x 104 -> 34 x 26, B=2  several tiles, ragged right and bottom, two images

dst starts from random values (not zero), so the state update old + sign * (acc + bias) is compared as well.

Block 20 (channel 256, stride 2) is the other caller of <64,64> / <64,256>: in bf16x3 its conv.4 and conv.7 go through
launch_pipe like those of the stride-1 blocks.  In f16x2h the same block runs on the fp16 kernels of conv3.hip, which do not
read the stage-3 options: that run is kept as a check that the options leave that path alone, it exercises no wide kernel.
"""
import ctypes as C

import pytest
import torch

from tests import block_ref as br
from tests import test_gpu_block_tiles as bt
from tests import test_gpu_parity as parity
from tests.zc import nchw_to_zc, ptr, stream
from vstnet_amd import _lib

pytestmark = pytest.mark.gpu

WIDE = {_lib.OPT_STAGE3_LEAN: 0, _lib.OPT_STAGE3_WIDE: 1}
EIGHT = {_lib.OPT_STAGE3_LEAN: 0, _lib.OPT_STAGE3_WIDE: 0}
SHAPES = [(16, 16, 1), (18, 10, 1), (34, 26, 2)]                     # (h, w, B) at quarter resolution
S1 = [br.Case("c256s1", 25, "stack.25.", 256, 1, h, w, B) for h, w, B in SHAPES]
S2 = br.Case("c256s2", 20, "stack.20.", 256, 2, 34, 26, 2)           # block 20: channel 256, stride 2
GUARD_BYTE = 0xA5
GUARD = 1 << 18                                                       # bytes in front of and behind each buffer (25 rows of dst)
ids = lambda cs: [c.id for c in cs]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    net, _, _ = parity.make_net("photo")                 # (the packed weights live as long as the net: it stays in this frame)
    yield _lib.lib(), net._ensure_packed(torch.device("cuda", torch.cuda.current_device()))


class Guarded:
    """`nbytes` of device memory with GUARD bytes of GUARD_BYTE on either side; `tail` more bytes of the buffer's own end are
    filled with the pattern too (the part of the block scratch behind h1 and h2, which no 256-channel bf16x3 block uses)"""

    def __init__(self, nbytes, tail=0):
        self.nbytes, self.tail = nbytes, tail
        self.raw = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.body = self.raw[GUARD:GUARD + nbytes]

    def intact(self):
        g = self.raw.cpu()
        return bool((g[:GUARD] == GUARD_BYTE).all() and (g[GUARD + self.nbytes - self.tail:] == GUARD_BYTE).all())


def apply(env, case, precision, direction, options, dst0, guarded=False):
    """dst0 (+/-)= F(src) of one block; returns dst (on the CPU) and whether every guard survived"""
    L, weights = env
    src = nchw_to_zc(br.case_src(case).float()).cuda()
    B, Hq, Wq = src.shape[0], src.shape[1], src.shape[2]
    H, W = 4 * Hq, 4 * Wq
    tmp_bytes = L.vst_block_tmp_bytes(B, H, W)
    used = 2 * B * (H >> 2) * (W >> 2) * 64 * 4                     # h1 and h2: 64 floats per quarter-resolution pixel each
    gd = Guarded(dst0.numel() * 4)
    gt = Guarded(tmp_bytes, tail=tmp_bytes - used if guarded else 0)
    if not guarded:
        gt.body.zero_()
    dst = gd.body.view(torch.float32).view(dst0.shape)
    dst.copy_(dst0)
    with bt._options(options):
        rc = L.vst_block_apply(C.byref(weights.blocks[case.k]), case.channel, case.stride, direction, bt.PREC[precision],
                               ptr(dst), ptr(src), ptr(gt.body), B, H, W, stream())
        _lib.check(rc, "vst_block_apply")
        torch.cuda.synchronize()
    return dst.cpu().clone(), gd.intact() and gt.intact()


def dst0_of(case):
    g = torch.Generator().manual_seed(case.seed + 7)
    Hq, Wq = case.frame[0] // 4, case.frame[1] // 4
    return torch.randn(case.B, Hq, Wq, 256, generator=g)


@pytest.mark.parametrize("case", S1, ids=ids(S1))
def test_wide_equals_eight_waves_both_directions(env, case):
    d0 = dst0_of(case)
    for direction in (+1, -1):
        wide, _ = apply(env, case, "bf16x3", direction, WIDE, d0)
        eight, _ = apply(env, case, "bf16x3", direction, EIGHT, d0)
        assert not torch.equal(wide, d0), "the block wrote nothing"
        assert torch.equal(wide.view(torch.int32), eight.view(torch.int32)), f"direction {direction}"


def test_wide_equals_eight_waves_block_20_bf16x3(env):
    """the stride-2 caller: conv.1 is a conv_mfma_kernel, conv.4 / conv.7 are conv_pipe_kernel<64,64> / <64,256> in the form the
    options select (136 x 104, B = 2: several ragged tiles)"""
    d0 = dst0_of(S2)
    for direction in (+1, -1):
        wide, _ = apply(env, S2, "bf16x3", direction, WIDE, d0)
        eight, _ = apply(env, S2, "bf16x3", direction, EIGHT, d0)
        assert not torch.equal(wide, d0), "the block wrote nothing"
        assert torch.equal(wide.view(torch.int32), eight.view(torch.int32)), f"direction {direction}"


def test_stage3_options_leave_block_20_f16x2h_alone(env):
    """f16x2h: block 20 runs on conv3.hip's fp16 kernels (run_block<256, 2>), not on conv_pipe_kernel; the options must not
    change a bit there"""
    d0 = dst0_of(S2)
    for direction in (+1, -1):
        wide, _ = apply(env, S2, "f16x2h", direction, WIDE, d0)
        eight, _ = apply(env, S2, "f16x2h", direction, EIGHT, d0)
        assert not torch.equal(wide, d0), "the block wrote nothing"
        assert torch.equal(wide.view(torch.int32), eight.view(torch.int32)), f"direction {direction}"


def test_no_stray_stores_on_the_ragged_frame(env):
    """72 x 40: guard bands around dst and the block scratch, and the scratch behind h1 / h2, keep their pattern after a forward
    and after an inverse call (a reordered store or a peeled stage that lands one row too far shows here and nowhere else)"""
    case = S1[1]
    d0 = dst0_of(case)
    for direction in (+1, -1):
        out, intact = apply(env, case, "bf16x3", direction, WIDE, d0, guarded=True)
        assert intact, f"direction {direction}: a guard band was written"
        assert torch.isfinite(out).all()


@pytest.mark.parametrize("case", S1, ids=ids(S1))
def test_wide_F_against_fp64(env, case):
    """the per-block bf16x3 bound of tests/test_gpu_block_tiles.py (2 x (model + e32), tests/block_ref.py), by its own check"""
    bt.check(case, "bf16x3", bt.ran(env, case, "bf16x3", WIDE), " [wide]")
