"""The high-bit-depth names under the module path they had before the two edges became one module, vstnet_amd/yuv.py, where they
live and are documented.  Nothing in this tree imports this path; it is kept because the test modules of the commit before the
merge do, and a path they import cannot go without taking those tests with it.  It holds no arithmetic of its own."""
from . import yuv
from .yuv import DEEP_TIE_EPS as TIE_EPS
from .yuv import (DeepYuvSpec, rgb_f32_to_yuv16, rgb_to_yuv16_float, rgb_to_yuv16_host, round_codes, yuv16_to_rgb_f32,  # noqa: F401
                  yuv16_to_rgb_float, yuv16_to_rgb_host)


def near_tie(v, eps=TIE_EPS):
    """yuv.near_tie with the deep epsilon as its default, as this path had it"""
    return yuv.near_tie(v, eps)
