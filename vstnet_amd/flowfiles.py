"""Host side of --temporal (video_transfer.py): optical-flow files in, the per-frame file and the closing line out.  Nothing here
touches a GPU.

A flow is float32 [2,H,W], x displacement first.  Middlebury .flo: the float32 magic 202021.25, int32 width, int32 height, then
H rows of W interleaved (u, v) float32 pairs, little-endian.  A .npy file holds the [2,H,W] array itself.

temporal.csv has one line per frame, in frame order: ``index,loss_out,loss_in`` - the temporal loss (the mean over the three
channels) of the stylised pair and of the input pair; the cells of a frame without a value (the first frame, a frame whose history
was stale) are empty.  Values are written with repr(), so a file read back and written again gives the same bytes.

stabilise.csv (--stabilise) has the same shape: ``index,loss_raw,loss_out`` - the temporal loss of the decoder's pair and of the
written, stabilised pair; its loss_out is temporal.csv's."""
import math
import os
import struct

import numpy as np

CSV_NAME = "temporal.csv"
STABILISE_CSV_NAME = "stabilise.csv"
FLO_MAGIC = 202021.25
FLOW_EXTENSIONS = (".flo", ".npy")


def write_flo(path, flow):
    f = np.asarray(flow)
    if f.ndim != 3 or f.shape[0] != 2:
        raise ValueError("%s: a flow is [2,H,W], got %s" % (path, (f.shape,)))
    h, w = f.shape[1:]
    with open(path, "wb") as out:
        out.write(struct.pack("<fii", FLO_MAGIC, w, h))
        out.write(np.ascontiguousarray(f.transpose(1, 2, 0)).astype("<f4").tobytes())
    return path


def read_flo(path):
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12:
        raise ValueError("%s: too short for a .flo header (%d bytes)" % (path, len(data)))
    magic, w, h = struct.unpack("<fii", data[:12])
    if magic != FLO_MAGIC:
        raise ValueError("%s: not a Middlebury .flo file (magic %r, expected %r)" % (path, magic, FLO_MAGIC))
    if w < 1 or h < 1 or len(data) != 12 + 8 * w * h:
        raise ValueError("%s: header says %dx%d, which needs %d bytes of flow; the file holds %d"
                         % (path, w, h, 8 * max(w, 0) * max(h, 0), len(data) - 12))
    uv = np.frombuffer(data, dtype="<f4", offset=12).reshape(h, w, 2)
    return np.ascontiguousarray(uv.transpose(2, 0, 1), dtype=np.float32)


def read_flow(path, hw=None, negate=False):
    """A .flo or .npy file as float32 [2,H,W]; with hw, a file of another size is an error that names it."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".flo":
        flow = read_flo(path)
    elif ext == ".npy":
        flow = np.load(path, allow_pickle=False)
        if flow.ndim != 3 or flow.shape[0] != 2:
            raise ValueError("%s: a flow is [2,H,W], got %s" % (path, (flow.shape,)))
        flow = np.ascontiguousarray(flow, dtype=np.float32)
    else:
        raise ValueError("%s: flow files are .flo or .npy" % path)
    if hw is not None and tuple(flow.shape[1:]) != (int(hw[0]), int(hw[1])):
        raise ValueError("%s: the flow is %dx%d, the stylised frames are %dx%d" % (path, flow.shape[2], flow.shape[1], hw[1], hw[0]))
    return -flow if negate else flow


def list_flows(flow_dir, n_frames):
    """The flow files of a clip of n_frames frames, sorted by name: one per frame transition."""
    if not os.path.isdir(flow_dir):
        raise ValueError("--flow_dir %s is not a directory" % flow_dir)
    names = sorted(f for f in os.listdir(flow_dir) if os.path.splitext(f)[1].lower() in FLOW_EXTENSIONS)
    if len(names) != n_frames - 1:
        raise ValueError("%s holds %d flow files (.flo / .npy); a clip of %d frames has %d transitions"
                         % (flow_dir, len(names), n_frames, n_frames - 1))
    return [os.path.join(flow_dir, f) for f in names]


def _cell(v):
    return "" if v is None or (isinstance(v, float) and math.isnan(v)) else repr(float(v))


def write_csv(path, per_frame, n_frames=None, valid=False):
    """per_frame: {frame index: (loss_out, loss_in)}; a missing frame (below n_frames), None or nan is an empty cell.  valid:
    the rows are (loss_out, loss_in, valid_share) and the file has a fourth column (--flow_mask)."""
    last = max(per_frame) + 1 if per_frame else 0
    n = 3 if valid else 2
    with open(path, "w") as f:
        for i in range(max(last, n_frames or 0)):
            f.write(",".join(["%d" % i] + [_cell(v) for v in per_frame.get(i, (None,) * n)[:n]]) + "\n")
    return path


def read_csv(path):
    """-> {frame index: (loss_out, loss_in)}, or (loss_out, loss_in, valid_share) for a file with the fourth column, with None
    for an empty cell"""
    rows = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            cells = line.rstrip("\n").split(",")
            if len(cells) not in (3, 4):
                raise ValueError("%s line %d: expected index,loss_out,loss_in[,valid], got %r" % (path, n, line.strip()))
            rows[int(cells[0])] = tuple(float(c) if c else None for c in cells[1:])
    return rows


def summary(per_frame):
    """The closing line: mean loss_out, mean loss_in, their ratio (how much the stylisation amplifies the input's own frame
    difference), the largest loss_out and its frame - over the frames that have both values; with a third value per row
    (--flow_mask) also the mean share of valid pixels."""
    vals = {i: v for i, v in per_frame.items()
            if all(x is not None and not math.isnan(x) for x in v)}
    if not vals:
        return "temporal: no frame pairs"
    out_m = sum(v[0] for v in vals.values()) / len(vals)
    in_m = sum(v[1] for v in vals.values()) / len(vals)
    worst = max(vals, key=lambda i: vals[i][0])
    ratio = "%.3f" % (out_m / in_m) if in_m > 0 else "inf"
    line = ("temporal (warping error, %d frame pairs): stylised mean %.6e, input mean %.6e, amplification %s, max %.6e (frame %d)"
            % (len(vals), out_m, in_m, ratio, vals[worst][0], worst))
    if all(len(v) == 3 for v in vals.values()):
        line += ", mean valid share %.4f" % (sum(v[2] for v in vals.values()) / len(vals))
    return line


def write_stabilise_csv(path, per_frame, n_frames=None):
    """per_frame: {frame index: (loss_raw, loss_out)}; a missing frame (below n_frames), None or nan is an empty cell."""
    last = max(per_frame) + 1 if per_frame else 0
    with open(path, "w") as f:
        for i in range(max(last, n_frames or 0)):
            f.write(",".join(["%d" % i] + [_cell(v) for v in per_frame.get(i, (None, None))[:2]]) + "\n")
    return path


def read_stabilise_csv(path):
    """-> {frame index: (loss_raw, loss_out)} with None for an empty cell"""
    rows = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            cells = line.rstrip("\n").split(",")
            if len(cells) != 3:
                raise ValueError("%s line %d: expected index,loss_raw,loss_out, got %r" % (path, n, line.strip()))
            rows[int(cells[0])] = tuple(float(c) if c else None for c in cells[1:])
    return rows


def stabilise_summary(per_frame):
    """The closing line of --stabilise: the mean loss of the decoder's pairs, of the written pairs, and their ratio - over the
    frames that have both values."""
    vals = [v for v in per_frame.values() if all(x is not None and not math.isnan(x) for x in v)]
    if not vals:
        return "stabilise: no frame pairs"
    raw_m = sum(v[0] for v in vals) / len(vals)
    out_m = sum(v[1] for v in vals) / len(vals)
    ratio = "%.3f" % (out_m / raw_m) if raw_m > 0 else "inf"
    return ("stabilise (warping error, %d frame pairs): decoded mean %.6e, written mean %.6e, written / decoded %s"
            % (len(vals), raw_m, out_m, ratio))
