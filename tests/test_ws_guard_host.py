"""What the workspace arena of tests/ws_guard.py rejects, shown on the CPU with small numpy "kernels" that take raw memory and a
byte offset the way a device kernel takes a pointer.  Each planted fault is one a workspace invites: a store one byte before the
workspace, at its end and at the far edge of the pad; a second stage that adds one partial more than the first stage wrote; a
second stage that reads one element past the workspace's end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ws_guard import PATTERNS, Arena, assert_placed, describe           # noqa: E402

PER_GROUP = 16                    # elements one "workgroup" of the first stage adds
X = np.random.default_rng(0).random(100)         # 7 groups, the last one ragged (4 elements)
GROUPS = -(-X.size // PER_GROUP)
WS_BYTES = 8 * GROUPS             # the "size function"


def mem(arena):
    """the arena's whole memory as numpy bytes: what a pointer can reach"""
    return arena.buf.numpy()


def partials_at(arena, count):
    """`count` doubles at the workspace's address, as a kernel would cast the pointer (no bounds: the pad is reachable)"""
    return np.frombuffer(mem(arena).data, dtype=np.float64, count=count, offset=arena.off)


def stage1(arena, groups=GROUPS):
    p = partials_at(arena, groups)
    for g in range(groups):
        p[g] = X[g * PER_GROUP:(g + 1) * PER_GROUP].sum()


def stage2(arena, count=GROUPS):
    total = np.float64(0.0)
    for v in partials_at(arena, count):             # in a fixed order, one partial after the other
        total = total + v
    return total


def reduce_correct(arena):
    stage1(arena)
    return stage2(arena)


def reduce_one_partial_more_than_written(arena):
    """the size function leaves room for GROUPS + 1 partials, the first stage writes GROUPS, the second adds GROUPS + 1: a stale
    read inside the workspace"""
    assert arena.bytes == WS_BYTES + 8
    stage1(arena)
    return stage2(arena, GROUPS + 1)


def reduce_reads_past_the_end(arena):
    """the second stage adds GROUPS + 1 partials: the last one lies in the pad"""
    stage1(arena)
    return stage2(arena, GROUPS + 1)


def three_fills(kernel, align=8):
    nbytes = WS_BYTES + (8 if kernel is reduce_one_partial_more_than_written else 0)
    outs = []
    for pat in PATTERNS:
        a = Arena(nbytes, align, "cpu", pad=256).fill(pat)
        with np.errstate(all="ignore"):
            outs.append(kernel(a))
        a.check(kernel.__name__)                    # (none of the reductions writes outside)
    return [np.float64(o).tobytes() for o in outs]


def test_placement():
    for align in (1, 4, 8, 16, 64, 256, 512):
        a = Arena(40, align, "cpu", pad=64)
        assert a.ptr == a.buf.data_ptr() + a.off and a.ptr % align == 0 and a.ptr % (2 * align) != 0
        assert a.ptr % 256 == align % 256 and a.bytes == 40 and a.ws().numel() == 40
        lo, hi = a.pads()
        assert lo.numel() == hi.numel() == 64 and hi.data_ptr() == a.ptr + 40 and lo.data_ptr() == a.ptr - 64
    assert Arena(0, 8, "cpu", pad=64).ws().numel() == 0


def test_placement_rejects_a_start_that_is_too_well_aligned():
    probe = Arena(40, 8, "cpu", pad=64)
    with pytest.raises(AssertionError, match="wanted 256 k \\+ 8"):
        Arena(40, 8, "cpu", pad=64, _start=probe.off + 8)             # 256 k + 16: a 16-byte-aligned start
    # (whatever address the allocator returns for the second tensor, the asserted rule itself says the same)
    with pytest.raises(AssertionError):
        assert_placed(0x1000 + 16, 8)
    with pytest.raises(AssertionError):
        assert_placed(0x1000, 256)                                    # 512-aligned
    assert_placed(0x1000 + 8, 8)
    assert_placed(0x1100, 256)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("where", ("-1", "bytes", "bytes+pad-1"))
def test_one_byte_written_outside_is_caught(where, pattern):
    a = Arena(WS_BYTES, 8, "cpu", pad=256).fill(pattern)
    off = {"-1": -1, "bytes": a.bytes, "bytes+pad-1": a.bytes + a.pad - 1}[where]
    stage1(a)
    a.check("clean")
    mem(a)[a.off + off] = pattern ^ 0x01            # the fault: one byte, one bit
    want = "first at offset -1, last at -1 relative to the start" if off < 0 else \
        f"first at offset {off - a.bytes:+d}, last at {off - a.bytes:+d} relative to the end"
    with pytest.raises(AssertionError) as e:
        a.check("planted")
    assert want in str(e.value) and "1 pad bytes written" in str(e.value), str(e.value)


def test_a_short_size_function_is_caught_with_its_offsets():
    """the workspace one partial short: the ragged group's partial lands in the pad, bytes 0..7 past the end"""
    a = Arena(WS_BYTES - 8, 8, "cpu", pad=256).fill(0xFF)
    stage1(a)
    with pytest.raises(AssertionError, match="first at offset \\+0, last at \\+7 relative to the end"):
        a.check("short")


def test_a_correct_reduction_passes_all_three_fills():
    outs = three_fills(reduce_correct)
    want = np.float64(0.0)
    for g in range(GROUPS):
        want = want + X[g * PER_GROUP:(g + 1) * PER_GROUP].sum()
    assert outs[0] == outs[1] == outs[2] == want.tobytes()


@pytest.mark.parametrize("kernel", (reduce_one_partial_more_than_written, reduce_reads_past_the_end))
def test_a_read_of_what_was_not_written_differs_under_every_fill(kernel):
    outs = three_fills(kernel)
    assert len(set(outs)) == 3, kernel.__name__     # NaN, huge, and - under zeros alone - the right answer
    assert outs[2] == three_fills(reduce_correct)[2]                  # which is why a fresh, zeroed block hides the fault


def test_touched_is_the_exact_range_of_a_known_write():
    a, b = Arena(64, 8, "cpu", pad=64).fill(0xFF), Arena(64, 8, "cpu", pad=64).fill(0x7F)
    assert a.touched(b) is None and describe(64, None) == "bytes 64 touched nothing tail 64"
    for arena in (a, b):
        m = mem(arena)
        m[arena.off + 5:arena.off + 41] = 0x7F      # the store's value is one pattern's own byte: invisible in b ...
        m[arena.off + 9:arena.off + 40] = 0x33
    assert a.touched(b) == (5, 40) == b.touched(a)  # ... and seen in a
    assert describe(64, a.touched(b)) == "bytes 64 touched [5, 40] tail 23"
    a.check()
    b.check()
    with pytest.raises(AssertionError):
        a.touched(Arena(64, 8, "cpu", pad=64).fill(0xFF))             # the same pattern twice shows nothing
    with pytest.raises(AssertionError):
        a.touched(Arena(64, 8, "cpu", pad=64).fill(0x00))


def test_fill_covers_workspace_and_pads():
    a = Arena(24, 16, "cpu", pad=32)
    for pat in PATTERNS:
        a.fill(pat)
        assert (a.ws().numpy() == pat).all() and all((p.numpy() == pat).all() for p in a.pads())
    assert isinstance(a.ptr, int) and torch.uint8 == a.buf.dtype
    with pytest.raises(AssertionError):
        a.fill(0x55)
