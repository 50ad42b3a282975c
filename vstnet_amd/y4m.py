"""YUV4MPEG2 (.y4m) files: the uncompressed interchange format ffmpeg, mpv, x264, x265, aomenc and SVT-AV1 read and write - a
text header, then per frame a `FRAME` line and the raw 8-bit planes Y, U, V.  Pure Python and numpy: a frame is read with one
readinto and written with one write; the colour conversion happens on the card (vstnet_amd/yuv.py).

Supported: progressive 8-bit C420jpeg, C420mpeg2, C420 (sited like C420jpeg) and C444.  Everything else raises, naming the token."""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from .yuv import YuvSpec

MAGIC = b"YUV4MPEG2"
LAYOUT_OF_TAG = {"420jpeg": "420jpeg", "420mpeg2": "420mpeg2", "420": "420jpeg", "444": "444"}
TAG_OF_LAYOUT = {"420jpeg": "C420jpeg", "420mpeg2": "C420mpeg2", "444": "C444"}
FRAME_LINE = b"FRAME\n"


class Y4MError(ValueError):
    pass


def auto_matrix(width, height):
    """what players assume of untagged material: BT.709 for HD sizes, BT.601 below"""
    return "bt709" if width >= 1280 or height > 576 else "bt601"


def _read_line(f, limit, what):
    """one '\\n'-terminated line of at most `limit` bytes, without the newline"""
    line = f.readline(limit + 1)
    if not line.endswith(b"\n"):
        raise Y4MError(f"{what}: no end of line within {limit} bytes")
    return line[:-1]


class Y4MClip:
    """A .y4m file as a lazy sequence, like video_transfer.FrameDir: len(), clip[i] (the frame's flat uint8 planes Y|U|V, a new
    array filled by one readinto), size = (width, height), fps (a Fraction), layout, colour_range ('limited' | 'full' | None:
    the header's XCOLORRANGE).  The frame index is built once by walking the FRAME lines - they may carry parameters - so access
    is random and a shard reads only its own frames."""

    def __init__(self, path):
        self.path = path
        self.layout, self.colour_range, self.fps = "420jpeg", None, Fraction(30, 1)
        width = height = None
        with open(path, "rb") as f:
            tokens = _read_line(f, 4096, f"{path}: header").split(b" ")
            if tokens[0] != MAGIC:
                raise Y4MError(f"{path}: not a YUV4MPEG2 file (it starts with {tokens[0][:16]!r})")
            for raw in tokens[1:]:
                if not raw:
                    continue
                tok = raw.decode("ascii", "replace")
                key, val = tok[0], tok[1:]
                if key == "W":
                    width = int(val)
                elif key == "H":
                    height = int(val)
                elif key == "F":
                    num, _, den = val.partition(":")
                    self.fps = Fraction(int(num), int(den or 1)) if int(num) > 0 and int(den or 1) > 0 else Fraction(30, 1)
                elif key == "I":
                    if val not in ("p", "?"):
                        raise Y4MError(f"{path}: header token {tok!r}: interlaced material is not supported (Ip or I? only)")
                elif key == "C":
                    if val not in LAYOUT_OF_TAG:
                        raise Y4MError(f"{path}: header token {tok!r}: only 8-bit C420jpeg, C420mpeg2, C420 and C444 are supported")
                    self.layout = LAYOUT_OF_TAG[val]
                elif key == "X":
                    if val.upper().startswith("COLORRANGE="):
                        rng = val.split("=", 1)[1].upper()
                        if rng not in ("FULL", "LIMITED"):
                            raise Y4MError(f"{path}: header token {tok!r}: XCOLORRANGE is FULL or LIMITED")
                        self.colour_range = rng.lower()
                # (A: the pixel aspect, and any other token: carried by the format, of no use here)
            if width is None or height is None or width < 1 or height < 1:
                raise Y4MError(f"{path}: the header lacks a positive W and H")
            self.size = (width, height)
            self.frame_bytes = YuvSpec(self.layout).frame_bytes(height, width)
            self.offsets = []
            end = os.fstat(f.fileno()).st_size
            pos = f.tell()
            while pos < end:
                i = len(self.offsets)
                line = f.readline(1025)
                if not line.startswith(b"FRAME") or not line.endswith(b"\n") or line[5:6] not in (b"\n", b" "):
                    raise Y4MError(f"{path}: frame {i}: no FRAME marker at byte {pos} (found {line[:12]!r})")
                pos += len(line)
                if pos + self.frame_bytes > end:
                    raise Y4MError(f"{path}: frame {i} is truncated: {end - pos} of {self.frame_bytes} bytes")
                self.offsets.append(pos)
                pos += self.frame_bytes
                f.seek(pos)

    def __len__(self):
        return len(self.offsets)

    def __getitem__(self, i):
        if not -len(self.offsets) <= i < len(self.offsets):
            raise IndexError(i)
        out = np.empty(self.frame_bytes, np.uint8)
        # (one descriptor per call: frames are read from several threads and processes)
        with open(self.path, "rb", buffering=0) as f:
            f.seek(self.offsets[i])
            if f.readinto(memoryview(out)) != self.frame_bytes:
                raise Y4MError(f"{self.path}: frame {i} is truncated")
        return out

    def spec(self, matrix="auto", colour_range="auto"):
        """the YuvSpec of the clip's frames: matrix auto = by size, range auto = the header's XCOLORRANGE, else limited"""
        m = auto_matrix(*self.size) if matrix == "auto" else matrix
        r = (self.colour_range or "limited") if colour_range == "auto" else colour_range
        return YuvSpec(self.layout, m, r)


def header_line(W, H, fps, spec):
    fps = Fraction(fps).limit_denominator(1001)
    return ("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s\n"
            % (W, H, fps.numerator, fps.denominator, TAG_OF_LAYOUT[spec.layout], spec.range.upper())).encode("ascii")


class Y4MWriter:
    """Frames in, one .y4m file out: the header, then FRAME\\n and the flat planes per frame.  header=False writes the frames
    alone (a shard's part, merge_parts puts the header in front)."""

    def __init__(self, path, W, H, fps, spec, header=True):
        self.path, self.frame_bytes, self.frames = path, spec.frame_bytes(H, W), 0
        self.f = open(path, "wb")
        if header:
            self.f.write(header_line(W, H, fps, spec))

    def write(self, flat):
        a = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
        if a.size != self.frame_bytes:
            raise ValueError(f"{self.path}: a frame is {self.frame_bytes} bytes, got {a.size}")
        self.f.write(FRAME_LINE)
        self.f.write(memoryview(a))
        self.frames += 1

    def close(self):
        if self.f is not None:
            self.f.close()
            self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def part_frames(n_frames, world):
    """frames per rank of a clip cut into `world` contiguous shards (vstnet_amd.sharding.shard_range)"""
    from .sharding import shard_range
    return [hi - lo for lo, hi in (shard_range(n_frames, r, world) for r in range(world))]


def _join_parts(path, header, parts, n_frames, per, remove):
    """header (may be empty), then the parts in rank order, in 4 MiB chunks.  Every part must hold exactly its shard's frames -
    frames x `per` bytes - or nothing is written.  The parts, and their directory if that empties it, are removed on request."""
    for r, (p, n) in enumerate(zip(parts, part_frames(n_frames, len(parts)))):
        if not os.path.exists(p):
            raise RuntimeError(f"merge: part {r} ({p}) is missing")
        have = os.path.getsize(p)
        if have != n * per:
            raise RuntimeError(f"merge: part {r} ({p}) holds {have} bytes, its {n} frames are {n * per}")
    with open(path, "wb") as out:
        out.write(header)
        for p in parts:
            with open(p, "rb") as f:
                while True:
                    chunk = f.read(1 << 22)
                    if not chunk:
                        break
                    out.write(chunk)
    if remove:
        for p in parts:
            os.remove(p)
        d = os.path.dirname(parts[0]) if parts else None
        if d and os.path.isdir(d) and not os.listdir(d):
            os.rmdir(d)
    return path


def merge_parts(path, parts, n_frames, W, H, fps, spec, remove=True):
    """The shards' headerless parts, in rank order, behind one header: the file one process writes.  Every part must hold
    exactly its shard's frames - frames x (6 + frame_bytes) bytes - or nothing is written."""
    return _join_parts(path, header_line(W, H, fps, spec), parts, n_frames, len(FRAME_LINE) + spec.frame_bytes(H, W), remove)
