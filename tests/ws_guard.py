"""A guarded arena for caller-provided workspaces: one uint8 tensor laid out as [pad | workspace | pad], the workspace of exactly
the stated size at exactly the stated minimum alignment, everything filled with one byte pattern before the call.

What it shows (tests/test_ws_guard_host.py plants each fault on the CPU):
  * a write outside [0, bytes): check() compares both pads with the pattern byte for byte and names the first and last changed
    offset, relative to the workspace's start (negative) or to its end (0 = the first byte past it);
  * a read of something the call did not write, inside the workspace or in a pad: the caller runs the call under 0xFF (a NaN in
    fp32 and fp64, -1 in every integer type), 0x7F (a huge finite float, a large positive integer) and 0x00 and compares the
    outputs bit for bit - a result that depends on such a read cannot agree under all three;
  * the bytes a call really uses: touched(other) is the lowest and highest offset at which this arena or `other`, which ran the
    same call under a different non-zero pattern, no longer holds its pattern (a kernel that happens to store one pattern's byte
    value cannot also store the other's).

Position: the workspace starts on `align` and on no coarser power of two - at a 256-byte boundary plus `align` for align < 256, at
an odd multiple of `align` otherwise - so a kernel that assumes more than the header promises meets an address that lacks it.
This module imports no GPU code; it works on CPU tensors as well."""
import numpy as np
import torch

PATTERNS = (0xFF, 0x7F, 0x00)


def assert_placed(addr, align):
    """addr lies on `align` and on no coarser power of two (for align < 256: a 256-byte boundary plus align)"""
    assert align >= 1 and align & (align - 1) == 0, align
    if align < 256:
        assert addr % 256 == align % 256, f"workspace at 256 k + {addr % 256}, wanted 256 k + {align}"
    assert addr % align == 0 and addr % (2 * align) == align, f"workspace at {addr:#x} is not on {align} and on nothing coarser"


class Arena:
    def __init__(self, nbytes, align, device, pad=65536, _start=None):
        nbytes, align, pad = int(nbytes), int(align), int(pad)
        assert nbytes >= 0 and pad >= 1
        grid = max(256, 2 * align)
        self.buf = torch.empty(pad + nbytes + pad + 2 * grid, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        if _start is None:                          # the first address >= base + pad that is grid k + align
            _start = pad + (align - (base + pad)) % grid
        self.off, self.bytes, self.align, self.pad = int(_start), nbytes, align, pad
        self.ptr = base + self.off
        self.pattern = None
        assert self.off >= pad and self.off + nbytes + pad <= self.buf.numel()
        assert_placed(self.ptr, align)

    # ---- views
    def ws(self):
        """the workspace's bytes (a view)"""
        return self.buf[self.off:self.off + self.bytes]

    def pads(self):
        return self.buf[self.off - self.pad:self.off], self.buf[self.off + self.bytes:self.off + self.bytes + self.pad]

    def fill(self, pattern):
        assert pattern in PATTERNS, pattern
        self.buf.fill_(pattern)
        self.pattern = pattern
        return self

    def _sync(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)

    # ---- checks
    def check(self, what=""):
        """both pads still hold the pattern, byte for byte"""
        assert self.pattern is not None, "fill() first"
        self._sync()
        lo, hi = (p.cpu().numpy() for p in self.pads())
        for side, a, origin in (("before the workspace's start", lo, -self.pad), ("past the workspace's end", hi, 0)):
            changed = np.nonzero(a != self.pattern)[0]
            assert changed.size == 0, (f"{what}: {changed.size} pad bytes written {side} (workspace of {self.bytes} bytes, fill "
                                       f"{self.pattern:#04x}): first at offset {int(changed[0]) + origin:+d}, last at "
                                       f"{int(changed[-1]) + origin:+d} relative to the {'end' if origin == 0 else 'start'}")

    def touched(self, other):
        """(low, high): the lowest and highest workspace offset that no longer holds its pattern here or in `other`; None when
        neither run wrote anything"""
        assert self.bytes == other.bytes and self.pattern and other.pattern and self.pattern != other.pattern, \
            "two arenas of one size under two different non-zero patterns"
        self._sync()
        other._sync()
        return _changed_range((self.ws() != self.pattern) | (other.ws() != other.pattern))


def _changed_range(mask, chunk=1 << 20):
    """(first, last) index of a true element of a 1-D bool tensor, None without one; chunk by chunk, so that a workspace of a
    gigabyte costs one flag per MiB on the host and not an index per byte"""
    n = mask.numel()
    flags = [bool(f) for a in range(0, n, chunk * 1024) for f in _chunk_flags(mask[a:a + chunk * 1024], chunk)]
    if not any(flags):
        return None
    lo, hi = flags.index(True), len(flags) - 1 - flags[::-1].index(True)
    first = lo * chunk + int(np.nonzero(mask[lo * chunk:(lo + 1) * chunk].cpu().numpy())[0][0])
    last = hi * chunk + int(np.nonzero(mask[hi * chunk:(hi + 1) * chunk].cpu().numpy())[0][-1])
    return first, last


def _chunk_flags(part, chunk):
    full = part.numel() // chunk * chunk
    flags = part[:full].view(-1, chunk).any(dim=1).cpu().tolist() if full else []
    return flags + ([bool(part[full:].any())] if part.numel() > full else [])


def describe(nbytes, rng):
    """'bytes 408 touched [0, 407] tail 0' - the figures DESIGN.md records"""
    if rng is None:
        return f"bytes {nbytes} touched nothing tail {nbytes}"
    return f"bytes {nbytes} touched [{rng[0]}, {rng[1]}] tail {nbytes - (rng[1] + 1)}"
