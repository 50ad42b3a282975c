"""Headerless raw YUV files (.yuv): what `ffmpeg -f rawvideo -pix_fmt yuv420p10le` writes and what HM, VTM, x265 and SVT-AV1
read - the planes Y, U, V of every frame, one frame after the other, nothing else.  Size, format and rate come from the command
line.  This is how high-bit-depth material arrives (the .y4m reader stays 8-bit: vstnet_amd/y4m.py); 8-bit 4:2:0 and 4:4:4 files
are read too.  Pure Python and numpy: a frame is read with one readinto and written with one write; the colour conversion
happens on the card (vstnet_amd/yuv.py)."""
from __future__ import annotations

import os
import re

import numpy as np

from .y4m import _join_parts, auto_matrix
from .yuv import DeepYuvSpec, YuvSpec

PIX_FMT = re.compile(r"^yuv(420|422|444)p(?:(9|10|12|14|16)le)?$")


def parse_pix_fmt(name):
    """'yuv420p' | 'yuv444p' | 'yuv4{20,22,44}p{9,10,12,14,16}le' -> (layout family '420' | '422' | '444', depth)"""
    m = PIX_FMT.match(name) if isinstance(name, str) else None
    if m is None or (m.group(2) is None and m.group(1) == "422"):
        raise ValueError(f"pix_fmt {name!r} is not supported: yuv420p, yuv444p, or yuv420p / yuv422p / yuv444p with 9, 10, 12, 14 or "
                         "16 bits, little-endian (e.g. yuv420p10le); 8-bit 4:2:2 and big-endian samples are not")
    return m.group(1), int(m.group(2) or 8)


def pix_fmt_spec(pix_fmt, size_wh, matrix="auto", colour_range="auto", siting="left"):
    """The spec of frames of this pix_fmt and size: a YuvSpec for 8-bit formats, a DeepYuvSpec otherwise.  Matrix auto: by size
    (y4m.auto_matrix); range auto: limited; siting ('left' | 'centre') applies to 4:2:0 only: 420mpeg2 | 420jpeg."""
    family, depth = parse_pix_fmt(pix_fmt)
    if siting not in ("left", "centre"):
        raise ValueError(f"siting is 'left' or 'centre', got {siting!r}")
    layout = family if family != "420" else ("420mpeg2" if siting == "left" else "420jpeg")
    m = auto_matrix(*size_wh) if matrix == "auto" else matrix
    r = "limited" if colour_range == "auto" else colour_range
    return YuvSpec(layout, m, r) if depth == 8 else DeepYuvSpec(layout, m, r, depth)


class RawYuvClip:
    """A raw .yuv file as a lazy sequence, like Y4MClip: len(), clip[i] (the frame's flat uint8 bytes Y|U|V, a new array filled by
    one readinto), size = (width, height), fps, pix_fmt, spec(matrix, colour_range).  A file that is not a whole number of
    frames is an error."""

    def __init__(self, path, width, height, pix_fmt, fps=30, siting="left"):
        self.path, self.size, self.pix_fmt, self.fps, self.siting = path, (int(width), int(height)), pix_fmt, fps, siting
        self.frame_bytes = pix_fmt_spec(pix_fmt, self.size, siting=siting).frame_bytes(self.size[1], self.size[0])
        total = os.path.getsize(path)
        if total % self.frame_bytes:
            raise ValueError(f"{path}: {total} bytes are not a whole number of {self.size[0]}x{self.size[1]} {pix_fmt} frames of "
                             f"{self.frame_bytes} bytes ({total % self.frame_bytes} bytes remain)")
        self.n = total // self.frame_bytes

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not -self.n <= i < self.n:
            raise IndexError(i)
        out = np.empty(self.frame_bytes, np.uint8)
        # (one descriptor per call: frames are read from several threads and processes)
        with open(self.path, "rb", buffering=0) as f:
            f.seek((i % self.n) * self.frame_bytes)
            if f.readinto(memoryview(out)) != self.frame_bytes:
                raise ValueError(f"{self.path}: frame {i} is truncated")
        return out

    def spec(self, matrix="auto", colour_range="auto"):
        return pix_fmt_spec(self.pix_fmt, self.size, matrix, colour_range, self.siting)


class RawYuvWriter:
    """Frames in, one raw file out: the flat bytes of every frame, one after the other (a shard's part looks the same)."""

    def __init__(self, path):
        self.path, self.frames = path, 0
        self.f = open(path, "wb")

    def write(self, flat):
        self.f.write(memoryview(np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)))
        self.frames += 1

    def close(self):
        if self.f is not None:
            self.f.close()
            self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def merge_parts(path, parts, n_frames, frame_bytes, remove=True):
    """The shards' parts, in rank order, one after the other: the file one process writes.  Every part must hold exactly its
    shard's frames - frames x frame_bytes bytes - or nothing is written."""
    return _join_parts(path, b"", parts, n_frames, frame_bytes, remove)
