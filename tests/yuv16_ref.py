"""The comparison rule and the cases for the high-bit-depth edge (include/vstnet.h, "High-bit-depth edge").  The arithmetic itself
lives in vstnet_amd/yuv.py (numpy, float64: the *_float functions give the unrounded values); this module adds the rule and
the helpers the tests share.

The rule: the device's codes, and the bytes of its u8 side output, must EQUAL floor(v64 + 0.5) of the reference's unrounded
values - every one of them.  That is decidable because the kernels compute in fp64: about ten operations on magnitudes up to
2^17 err by under 2^-32, so a device value and the reference can fall on different sides of a tie only when the reference lies
within that of one.  Every case is therefore required to hold no value within 2^-20 of a rounding tie - a condition of the case,
checked on the CPU on the reference alone and asserted inside the test; random cases are chosen by seed until it holds (with at
most about 1.5e5 values per case the expected number of near-tie values is about 0.3 per seed: a qualifying seed is among the
first few).  No value is then left out of the comparison.  A rounding tie is a value k + 1/2 whose two neighbours k and k + 1
are both codes: at 2^depth - 1/2 and above, and at -1/2 and below, either side of the "tie" clamps to the same code, so those
values decide nothing and do not count (full-range chroma of a saturated blue or red is exactly 2^depth - 1/2).  The fp32
planes of yuv16_to_rgb_f32 must lie within one fp32 spacing of the float64 value: one rounding of an accurate value."""
import itertools

import numpy as np

from vstnet_amd import yuv
from vstnet_amd.yuv import DEEP_TIE_EPS as TIE_EPS  # noqa: F401
from vstnet_amd.yuv import (DeepYuvSpec, rgb_to_yuv16_float, rgb_to_yuv16_host, round_codes, yuv16_to_rgb_float,  # noqa: F401
                            yuv16_to_rgb_host)
from yuv_ref import KERNEL_SHAPES  # noqa: F401

LAYOUTS, MATRICES, RANGES = ("444", "422", "420jpeg", "420mpeg2"), ("bt601", "bt709"), ("limited", "full")
SPECS_10 = [DeepYuvSpec(l, m, r, 10) for l, m, r in itertools.product(LAYOUTS, MATRICES, RANGES)]
SPECS_DEPTHS = [DeepYuvSpec(l, "bt709", "limited", d) for d in (9, 12, 14, 16) for l in LAYOUTS]
DEPTH_SHAPES = [(3, 5), (9, 13), (55, 97)]


def near_tie(v, eps=TIE_EPS):
    """yuv.near_tie with the deep epsilon as its default"""
    return yuv.near_tie(v, eps)


def shapes_of(spec):
    return KERNEL_SHAPES if spec.depth == 10 else DEPTH_SHAPES


def deciding_ties(v64, top):
    """where v lies within 2^-20 of a tie between two values of 0..top (outside, both sides clamp to the same value)"""
    v64 = np.asarray(v64, np.float64)
    return near_tie(v64) & (v64 > 0.0) & (v64 < float(top))


def assert_tie_free(v64, what, top=255):
    """the condition of a case: no reference value within 2^-20 of a rounding tie"""
    tie = deciding_ties(v64, top)
    assert not tie.any(), f"{what}: {int(tie.sum())} reference values lie within 2^-20 of a tie: not a valid case"


def check_rgb(got_f32, got_u8, v64, what):
    """yuv16_to_rgb_f32's outputs against the unrounded, clamped float64 [H, W, 3] on the 0..1 scale.  got_f32: [3, H, W];
    got_u8: [H, W, 3] or None.  Returns the largest fp32 error in spacings, for a test to print."""
    v64 = np.asarray(v64, np.float64)
    assert_tie_free(255.0 * v64, what + " (u8)")
    got = np.asarray(got_f32).transpose(1, 2, 0)
    assert got.dtype == np.float32 and got.shape == v64.shape, (what, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - v64)
    ulp = np.spacing(v64.astype(np.float32)).astype(np.float64)
    assert (err <= ulp).all(), f"{what}: an fp32 value is {float((err / ulp).max()):.3f} spacings from the float64 value"
    if got_u8 is not None:
        want = np.floor(255.0 * v64 + 0.5).astype(np.uint8)
        got_u8 = np.asarray(got_u8)
        assert got_u8.dtype == np.uint8 and got_u8.shape == want.shape, (what, got_u8.dtype, got_u8.shape)
        bad = got_u8 != want
        assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ, first at {np.argwhere(bad)[0]}: {got_u8[bad][0]} for " \
                              f"{255.0 * v64[bad][0]!r}"
    return float((err / ulp).max())


def check_codes(got_u16, v64, spec, what):
    """vst_rgb_f32_to_yuv16's codes (flat uint16 Y|U|V) against the unrounded float64 codes"""
    got, v64 = np.asarray(got_u16), np.asarray(v64, np.float64)
    assert got.dtype == np.uint16 and got.shape == v64.shape, (what, got.dtype, got.shape, v64.shape)
    assert_tie_free(v64, what, spec.max_code)
    want = round_codes(v64, spec)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} codes differ, first at {np.argwhere(bad)[0]}: {got[bad][0]} for {v64[bad][0]!r}"


def tie_free_seed(make, values, top, first=0, tries=200):
    """the first seed >= first for which values(make(seed)) holds no near-tie value between two values of 0..top"""
    for seed in range(first, first + tries):
        if not deciding_ties(values(make(seed)), top).any():
            return seed
    raise AssertionError("no tie-free seed found")


def as_flat(codes_u16):
    """uint16 codes -> the flat little-endian bytes of a frame"""
    return np.ascontiguousarray(codes_u16, dtype="<u2").view(np.uint8)


def random_planes(spec, H, W, seed):
    """one flat frame Y|U|V of random codes below 2^depth, as bytes"""
    n = spec.frame_bytes(H, W) // 2
    return as_flat(np.random.default_rng(seed).integers(0, spec.max_code + 1, n, dtype=np.uint16))


def out_of_range_planes(spec, H, W, seed):
    """limited range: luma codes outside the nominal range and chroma at the extremes, so that the [0, 1] clamp fires"""
    n, s = spec.frame_bytes(H, W) // 2, 1 << (spec.depth - 8)
    rng = np.random.default_rng(seed)
    out = np.empty(n, np.uint16)
    out[:H * W] = rng.choice(np.r_[0:16 * s, 236 * s:spec.max_code + 1], H * W)
    out[H * W:] = rng.choice([0, spec.max_code], n - H * W)
    return as_flat(out)


def planes_cases(spec, H, W):
    """[(name, flat frame bytes)] for vst_yuv16_to_rgb_f32 at one shape.  The u8 side output is what rounds: the tie condition is
    on 255 v."""
    def values(flat):
        return 255.0 * yuv16_to_rgb_float(flat, H, W, spec)
    n = spec.frame_bytes(H, W) // 2
    seed = tie_free_seed(lambda s: random_planes(spec, H, W, s), values, 255, 7 * H + W)
    cases = [("random", random_planes(spec, H, W, seed)), ("zeros", as_flat(np.zeros(n, np.uint16))),
             ("max code", as_flat(np.full(n, spec.max_code, np.uint16))), ("0xFFFF", as_flat(np.full(n, 0xFFFF, np.uint16)))]
    if spec.range == "limited":
        seed = tie_free_seed(lambda s: out_of_range_planes(spec, H, W, s), values, 255, 7 * H + W + 1)
        cases.append(("out of range", out_of_range_planes(spec, H, W, seed)))
    return cases


def random_rgb(H, W, seed):
    """float32 [H, W, 3] in [-0.25, 1.25]: both clamps fire on every channel.  A pixel whose three channels ALL clamp is a corner
    of the RGB cube, and there full-range chroma is exactly -1/2 or +1/2 of its scale - yellow's Cb and cyan's Cr are the code
    1/2 exactly, a true tie that no seed avoids once a case has a few hundred pixels (one pixel in 27 is a corner) - so such a
    pixel has its red drawn again inside (0, 1).  Black and white are the fixed cases."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.25, 1.25, (H, W, 3))
    corner = ((a < 0.0) | (a > 1.0)).all(axis=-1)
    a[corner, 0] = rng.uniform(0.05, 0.95, int(corner.sum()))
    return a.astype(np.float32)


def rgb_cases(spec, H, W):
    """[(name, float32 [H, W, 3])] for vst_rgb_f32_to_yuv16 at one shape"""
    seed = tie_free_seed(lambda s: random_rgb(H, W, s), lambda a: rgb_to_yuv16_float(a, spec), spec.max_code, 11 * H + W)
    return [("random", random_rgb(H, W, seed)), ("zeros", np.zeros((H, W, 3), np.float32)), ("ones", np.ones((H, W, 3), np.float32))]


def write_raw(path, frames):
    """a raw .yuv file from flat frames, written by hand (not by RawYuvWriter: the reader's tests must not depend on the writer)"""
    with open(path, "wb") as f:
        for fr in frames:
            f.write(np.asarray(fr, np.uint8).tobytes())
    return path
