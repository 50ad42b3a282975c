"""The float64 restatement of the raw video edge's arithmetic (include/vstnet.h, "Raw video edge") and the comparison rule
for the fp32 kernels.  The arithmetic itself lives in vstnet_amd/yuv.py (numpy, float64: the *_float functions give the
unrounded values); this module adds the rule and the helpers the tests share.

The rule: a device byte must equal floor(v64 + 0.5) where |frac(v64) - 1/2| >= 2^-10, and may differ by one count elsewhere.
fp32 evaluation of these expressions on magnitudes <= 512 errs by under 6e-5 (a float32 restatement over all 8 layout x matrix
x range combinations at 8x8, 9x13 and 36x52 changed no byte); 2^-10 is about 18 times that.  The share of near-tie bytes is a
condition of a case, asserted on the reference alone: at most 2 %."""
import itertools

import numpy as np

from vstnet_amd.yuv import (TIE_EPS, YuvSpec, near_tie, rgb_to_yuv_float, rgb_to_yuv_host, round_bytes,  # noqa: F401
                            yuv_to_rgb_float, yuv_to_rgb_host)

LAYOUTS, MATRICES, RANGES = ("444", "420jpeg", "420mpeg2"), ("bt601", "bt709"), ("limited", "full")
ALL_SPECS = [YuvSpec(*c) for c in itertools.product(LAYOUTS, MATRICES, RANGES)]
MAX_TIE_SHARE = 0.02


def check_bytes(got, v64, what=""):
    """The comparison rule.  got: the device's bytes; v64: the unrounded float64 values, same shape.  Returns (near-tie share,
    bytes that differ) for a test to print."""
    got, v64 = np.asarray(got), np.asarray(v64, np.float64)
    assert got.shape == v64.shape and got.dtype == np.uint8, (what, got.shape, v64.shape, got.dtype)
    want = round_bytes(v64)
    tie = near_tie(v64) & (v64 > -0.5 - TIE_EPS) & (v64 < 255.5 + TIE_EPS)      # (clamped values have no tie)
    share = float(tie.mean()) if tie.size else 0.0
    assert share <= MAX_TIE_SHARE, f"{what}: {100 * share:.2f} % of the reference's bytes sit within 2^-10 of a tie"
    diff = got.astype(np.int16) - want.astype(np.int16)
    bad = (diff != 0) & ~tie
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ away from a tie, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][0]} for {v64[bad][0]!r}"
    assert np.abs(diff).max(initial=0) <= 1, f"{what}: a near-tie byte differs by {int(np.abs(diff).max())} counts"
    return share, int((diff != 0).sum())


def tie_free_seed(make, values, first=0, tries=200):
    """the first seed >= first for which values(make(seed)) holds no near-tie value: for the very small shapes, where one
    near-tie byte is already more than 2 %"""
    for seed in range(first, first + tries):
        if not near_tie(values(make(seed))).any():
            return seed
    raise AssertionError("no tie-free seed found")


def random_planes(spec, H, W, seed):
    """one flat frame Y|U|V of random bytes"""
    return np.random.default_rng(seed).integers(0, 256, spec.frame_bytes(H, W), dtype=np.uint8)


def random_rgb(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def write_y4m(path, frames, W, H, tag="C420mpeg2", extra="", frame_params=""):
    """a .y4m file from flat frames, written by hand (not by Y4MWriter: the reader's tests must not depend on the writer)"""
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F25:1 Ip A1:1%s%s\n" % (W, H, " " + tag if tag else "", extra)).encode())
        for fr in frames:
            f.write(b"FRAME" + frame_params.encode() + b"\n")
            f.write(np.asarray(fr, np.uint8).tobytes())
    return path


KERNEL_SHAPES = [(1, 1), (2, 2), (3, 5), (9, 13), (36, 52), (55, 97), (64, 260)]      # (H, W)


def _tiny(H, W):
    return H * W <= 15          # one near-tie byte would already be more than 2 % of the case


def planes_cases(spec, H, W):
    """[(name, flat planes)] for vst_yuv_to_rgb_u8 at one shape: random bytes (tiny shapes: a seed whose reference has no
    near-tie byte), all 0, all 255 and - limited range - planes of out-of-range codes only, so that both clamps fire"""
    seed = 7 * H + W
    if _tiny(H, W):
        seed = tie_free_seed(lambda s: random_planes(spec, H, W, s), lambda f: yuv_to_rgb_float(f, H, W, spec), seed)
    n = spec.frame_bytes(H, W)
    cases = [("random", random_planes(spec, H, W, seed)), ("zeros", np.zeros(n, np.uint8)), ("255s", np.full(n, 255, np.uint8))]
    if spec.range == "limited":
        rng = np.random.default_rng(seed + 1)
        out = np.empty(n, np.uint8)
        out[:H * W] = rng.choice(np.r_[0:16, 236:256], H * W)
        out[H * W:] = rng.choice([0, 255], n - H * W)
        cases.append(("out of range", out))
    return cases


def rgb_cases(spec, H, W):
    """[(name, uint8 [H, W, 3])] for vst_rgb_to_yuv_u8 at one shape"""
    seed = 11 * H + W
    if _tiny(H, W):
        seed = tie_free_seed(lambda s: random_rgb(H, W, s), lambda a: rgb_to_yuv_float(a, spec), seed)
    return [("random", random_rgb(H, W, seed)), ("zeros", np.zeros((H, W, 3), np.uint8)), ("255s", np.full((H, W, 3), 255, np.uint8))]
