"""The antialiased float resize on the card (csrc/resize.hip: vst_resize_f32, vst_resize_f32_to_u8 - resize_h_kernel<F32Arith, 1,
128>, resize_v_f32_kernel, resize_v_f32_u8_kernel), through the C ABI, element by element against the float64 reference of
tests/resize_f32_ref.py and its bound E, at the shapes where the kernels' indexing can go wrong.  B = 2 throughout, so that
plane and image indexing count; outputs and the pass buffer sit between sentinel guards, the pass buffer starts as NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import resize_f32_ref as R
from tests.test_gpu_color import Guarded
from vstnet_amd import _lib

pytestmark = pytest.mark.gpu

REACHES = ["upscale, frame far smaller than one tile",
           "Hs = 9: row groups of 8 straddle planes; Wd one short of the tile",
           "two 128-column tiles and a tail; a second 256-column block of the vertical pass",
           "shrink 16 in both axes, ksize 65, the largest LDS image",
           "one source pixel; the output is that pixel",
           "horizontal only",
           "vertical only, no tmp",
           "3 Wd = 1029: a second block of the byte pass; rowbytes % 4 = 1, rows alternate between the dword store and the byte tail",
           "vertical ksize 29 on a 19-wide row"]
IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.CASES]
assert len(REACHES) == len(R.CASES)


def call(i, to_u8, out_offset=0):
    """one call on CASES[i] -> the output as numpy ([B,3,Hd,Wd] float32 or [B,Hd,Wd,3] uint8); guards checked here"""
    from vstnet_amd.resize import _tables_on
    x, _, _ = R.case(i)
    (Hs, Ws), (Hd, Wd) = R.CASES[i]
    B = x.shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    tables = _tables_on("f32", dev, ([(Ws, Wd)] if Ws != Wd else []) + [(Hs, Hd)])
    xg = Guarded(x.size, torch.float32, data=x)
    og = Guarded(B * 3 * Hd * Wd, torch.uint8 if to_u8 else torch.float32, out_offset)
    tg = None
    if Ws != Wd:
        tg = Guarded(B * 3 * Hs * Wd, torch.float32)
        tg.view.fill_(float("nan"))
    fn = _lib.lib().vst_resize_f32_to_u8 if to_u8 else _lib.lib().vst_resize_f32
    st = torch.cuda.current_stream()
    rc = fn(xg.ptr, B, Hs, Ws, og.ptr, Hd, Wd, C.c_void_p(tables.data_ptr()), tg.ptr if tg else None, C.c_void_p(st.cuda_stream))
    st.synchronize()
    assert rc == 0, rc
    assert og.guards_intact(), f"{IDS[i]}: elements outside the output were written"
    assert xg.guards_intact() and (tg is None or tg.guards_intact()), f"{IDS[i]}: elements outside the pass buffer were written"
    if tg is not None:
        assert bool(torch.isfinite(tg.view).all()), f"{IDS[i]}: the pass buffer was not written everywhere"
    return og.host().reshape((B, Hd, Wd, 3) if to_u8 else (B, 3, Hd, Wd))


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_float_form_against_float64(i):
    _, ref, e = R.case(i)
    got = call(i, False)
    ok, worst = R.check_float(got, ref, e)
    print(f"vst_resize_f32 {IDS[i]} ({REACHES[i]}): worst error / E {worst:.3f}")
    assert ok.all(), (int((~ok).sum()), worst)
    if R.CASES[i][0] == (1, 1):
        x = R.case(i)[0]
        assert np.array_equal(got, np.broadcast_to(x, got.shape))


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_byte_form_against_float64(i):
    """within one count of trunc(clamp(255 ref)), differing only where 255 ref is within 255 E + 255 |ref| u of an integer; once
    more with the output one byte past an aligned base: the same bytes"""
    _, ref, e = R.case(i)
    got = call(i, True)
    ok, differ, maxd = R.check_bytes(got, ref, e)
    print(f"vst_resize_f32_to_u8 {IDS[i]}: {differ} of {got.size} bytes differ from the reference's (max {maxd})")
    assert ok.all() and maxd <= 1, (int((~ok).sum()), maxd)
    assert np.array_equal(call(i, True, out_offset=1), got)
