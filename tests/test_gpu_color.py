"""The Lab luminance blend on the card (csrc/color.hip: vst_lab_luminance, vst_lab_luminance_u8, vst_lab_luminance_u8_f32),
through the C ABI, element by element against the float64 reference of tests/color_ref.py with its running bound A + P * Bp
(P = color_ref.P_ASSERT; no tolerance here comes from a device run).  Every input set is laid out in every shape and base that
selects a code path, outputs go into sentinel-filled buffers with guards on both sides, and each test prints the worst
error / bound and P_needed, the smallest P at which all of its elements pass."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import color_ref as R
from vstnet_amd import _lib

pytestmark = pytest.mark.gpu
T = torch.from_numpy

SETS = ("uniform", "dark", "knees", "gamut", "bytes", "identity")
PAD = 64                               # guard elements: 256 bytes of floats, 64 bytes of uint8 - an aligned base stays aligned
SENTINEL = {torch.float32: -777.25, torch.uint8: 0xA5}

# (B, H, W), which buffer sits one element past an aligned base
LAYOUTS = [((1, 1, 1), None),          # smallest frame
           ((1, 7, 13), None),         # scalar form, one workgroup
           ((3, 33, 50), None),        # scalar, n % 4 == 2, batch in blockIdx.y
           ((2, 64, 64), None),        # vector form
           ((2, 36, 60), None),        # vector form with a ragged last workgroup: n / 4 = 540
           ((2, 64, 64), "content"),   # the scalar fallback at n % 4 == 0, by each base in turn
           ((2, 64, 64), "stylised"),
           ((2, 64, 64), "out")]


class Guarded:
    """a device view of n elements, `offset` elements past an aligned base, in a sentinel-filled buffer with PAD guard elements
    on both sides (after tests/test_gpu_yuv.py's Guarded)"""

    def __init__(self, n, dtype, offset=0, data=None):
        self.n, self.lo = n, PAD + offset
        self.buf = torch.full((self.lo + n + PAD,), SENTINEL[dtype], dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf[self.lo:self.lo + n]
        if data is not None:
            self.view.copy_(T(np.array(data).reshape(-1)))             # (a writable copy: the sets are read-only)
        self.fill = SENTINEL[dtype]

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def guards_intact(self):
        h = self.buf.cpu()
        return bool((h[:self.lo] == self.fill).all()) and bool((h[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf.cpu() == self.fill).all())

    def host(self):
        return self.view.cpu().numpy()


ENTRY = {"f32": ("vst_lab_luminance", "f32", torch.float32), "u8_f32": ("vst_lab_luminance_u8_f32", "u8", torch.float32),
         "u8": ("vst_lab_luminance_u8", "u8", torch.uint8)}


def layout_index(n_set, shape, k):
    """which pixels of a set a frame of `shape` holds: consecutive ones from a start that differs per layout"""
    B, H, W = shape
    return (np.arange(B * H * W) + 7919 * k) % n_set


def full_layouts(n_set):
    """the whole set once in the scalar form (n % 4 != 0) and once in the vector form (n % 4 == 0, the tail repeats)"""
    odd = n_set if n_set % 4 else n_set + 1
    return [((1, 1, odd), None), ((1, 1, (n_set + 3) // 4 * 4), None)]


def run(entry, c, s, shape, mis=None, in_place=False, stream=None):
    """one call: c [B n, 3] (float32 or uint8), s [B n, 3] float32 in pixel order -> the output in pixel order [B n, 3]; the
    guards of the output are checked here"""
    name, cmode, odtype = ENTRY[entry]
    B, H, W = shape
    n = H * W
    planes = lambda a: np.ascontiguousarray(a.reshape(B, n, 3).transpose(0, 2, 1))          # noqa: E731
    cg = Guarded(3 * B * n, torch.uint8 if cmode == "u8" else torch.float32, int(mis == "content"), c if cmode == "u8" else planes(c))
    sg = Guarded(3 * B * n, torch.float32, int(mis == "stylised"), planes(s))
    og = sg if in_place else Guarded(3 * B * n, odtype, int(mis == "out"))
    if mis is not None:
        g = {"content": cg, "stylised": sg, "out": og}[mis]
        assert g.view.data_ptr() % (4 if g.view.dtype == torch.uint8 else 16) != 0
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()                                   # the buffers were filled on the current stream
    rc = getattr(_lib.lib(), name)(cg.ptr, sg.ptr, og.ptr, B, H, W, C.c_void_p(st.cuda_stream))
    st.synchronize()
    assert rc == 0, (name, shape, rc)
    assert og.guards_intact(), f"{name} {shape} {mis}: elements outside the output were written"
    assert cg.guards_intact() and (in_place or sg.guards_intact())
    out = og.host()
    return out.reshape(B, n, 3).reshape(-1, 3) if odtype == torch.uint8 else out.reshape(B, 3, n).transpose(0, 2, 1).reshape(-1, 3)


def layouts_of(name, mode):
    c, s, ref = R.case(name, mode)
    for k, (shape, mis) in enumerate(LAYOUTS + full_layouts(len(s))):
        idx = layout_index(len(s), shape, k if k < len(LAYOUTS) else 0)
        yield shape, mis, c[idx], s[idx], ref.take(idx)


@pytest.mark.parametrize("entry", ["f32", "u8_f32"])
def test_float_forms_against_float64(entry):
    """every element within A + P * Bp of some variant of the reference, P = 2"""
    failed = []
    for name in SETS:
        worst, p_needed, count = 0.0, 0.0, 0
        for shape, mis, c, s, ref in layouts_of(name, ENTRY[entry][1]):
            ok, w, p = R.check_float(run(entry, c, s, shape, mis), ref)
            worst, p_needed, count = max(worst, w), max(p_needed, p), count + ok.size
            if not ok.all():
                failed.append((name, shape, mis, int((~ok).sum()), w, p))
        print(f"{ENTRY[entry][0]} {name}: {count} elements, worst error / bound {worst:.3f}, P_needed {p_needed:.3f}")
    assert not failed, failed


def test_byte_form_against_float64():
    """every byte within one count of the reference's byte, and different from it only where 255 * ref lies within 255 * bound
    of an integer, for some variant: a condition on every byte, not a share"""
    failed = []
    for name in SETS:
        differ, count = 0, 0
        for shape, mis, c, s, ref in layouts_of(name, "u8"):
            ok, d, maxd = R.check_bytes(run("u8", c, s, shape, mis), ref)
            differ, count = differ + d, count + ok.size
            if not ok.all() or maxd > 1:
                failed.append((name, shape, mis, int((~ok).sum()), maxd))
        print(f"vst_lab_luminance_u8 {name}: {count} bytes, {differ} differ from the reference's byte (each by one, each allowed)")
    assert not failed, failed


@pytest.mark.parametrize("entry", ["f32", "u8_f32"])
def test_in_place_gives_the_same_bits(entry):
    for name in ("uniform", "gamut"):
        c, s, _ = R.case(name, ENTRY[entry][1])
        for k, (shape, mis) in enumerate(LAYOUTS):
            if mis == "out":
                continue
            idx = layout_index(len(s), shape, k)
            want = run(entry, c[idx], s[idx], shape, mis)
            got = run(entry, c[idx], s[idx], shape, mis, in_place=True)
            assert got.tobytes() == want.tobytes(), (name, shape, mis)


@pytest.mark.parametrize("entry", ["f32", "u8_f32", "u8"])
def test_two_calls_give_the_same_bits(entry):
    other = torch.cuda.Stream()
    c, s, _ = R.case("uniform", ENTRY[entry][1])
    for k, (shape, mis) in enumerate(LAYOUTS):
        idx = layout_index(len(s), shape, k)
        a = run(entry, c[idx], s[idx], shape, mis)
        b = run(entry, c[idx], s[idx], shape, mis, stream=other)
        assert a.tobytes() == b.tobytes(), (shape, mis)


@pytest.mark.parametrize("entry", ["f32", "u8_f32", "u8"])
def test_non_finite_stylised_values(entry):
    """clamp_01 is fminf(fmaxf(v, 0), 1): a NaN in the stylised planes acts as 0, +Inf as 1, -Inf as 0.  The output is the
    output for the substituted finite value bit for bit, and the other pixels of the same thread's quad are what they were."""
    c, s, _ = R.case("uniform", ENTRY[entry][1])
    for k, (shape, mis) in enumerate(LAYOUTS[1:5]):                    # scalar and vector forms
        idx = layout_index(len(s), shape, k)
        ci, clean = c[idx], s[idx].copy()
        n_px = len(clean)
        spots = [(5 % n_px, 0), (6 % n_px, 2), (n_px - 1, 1), (n_px // 2, 0), (n_px // 2, 1), (n_px // 2, 2)]
        base = run(entry, ci, clean, shape, mis)
        for bad, sub in ((np.nan, 0.0), (np.inf, 1.0), (-np.inf, 0.0)):
            dirty, fixed = clean.copy(), clean.copy()
            for p, ch in spots:
                dirty[p, ch], fixed[p, ch] = bad, sub
            got, want = run(entry, ci, dirty, shape, mis), run(entry, ci, fixed, shape, mis)
            assert got.tobytes() == want.tobytes(), (shape, bad)
            assert np.isfinite(got.astype(np.float64)).all()
            touched = np.zeros(n_px, bool)
            touched[[p for p, _ in spots]] = True
            assert got[~touched].tobytes() == base[~touched].tobytes(), (shape, bad)     # quad neighbours included


def test_refusals_launch_nothing():
    L = _lib.lib()
    big = 32768                        # 2^30 pixels: past both limits (2^26 at the byte edge, (2^31 - 1) / 4 for float content)
    for entry, (name, cmode, odtype) in ENTRY.items():
        fn = getattr(L, name)
        n = 16
        cg = Guarded(3 * n, torch.uint8 if cmode == "u8" else torch.float32, data=np.zeros(3 * n, np.uint8 if cmode == "u8" else np.float32))
        sg = Guarded(3 * n, torch.float32, data=np.full(3 * n, 0.5, np.float32))
        og = Guarded(3 * n, odtype)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert fn(None, sg.ptr, og.ptr, 1, 4, 4, st) == -1
        assert fn(cg.ptr, None, og.ptr, 1, 4, 4, st) == -1
        assert fn(cg.ptr, sg.ptr, None, 1, 4, 4, st) == -1
        assert fn(cg.ptr, sg.ptr, og.ptr, 0, 4, 4, st) == -2
        assert fn(cg.ptr, sg.ptr, og.ptr, 65536, 4, 4, st) == -2
        assert fn(cg.ptr, sg.ptr, og.ptr, 1, big, big, st) == -2
        assert fn(cg.ptr, sg.ptr, og.ptr, 1, 0, 4, st) == -2 and fn(cg.ptr, sg.ptr, og.ptr, 1, 4, -1, st) == -2
        if cmode == "u8":
            assert fn(cg.ptr, sg.ptr, og.ptr, 1, 8192, 8193, st) == -2          # one row past VST_MAX_FRAME_PIXELS
        else:
            assert fn(cg.ptr, sg.ptr, og.ptr, 1, 23171, 23171, st) == -2        # 23171^2 > (2^31 - 1) / 4
        torch.cuda.synchronize()
        assert og.untouched(), name
        assert fn(cg.ptr, sg.ptr, og.ptr, 1, 4, 4, st) == 0                     # the same buffers are taken once the shape is right
        torch.cuda.synchronize()
        assert og.guards_intact() and not og.untouched()
