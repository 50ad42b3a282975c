"""Host side of --affinity (video_transfer.py, image_transfer.py): the per-frame file, the join of the shards' parts and the
closing line.  Nothing here touches a GPU.

affinity.csv has one line per frame, in frame order: ``index,loss_work`` or, under --upscale guided, ``index,loss_work,loss_full``
- the Matting-Laplacian loss (the sum over the three channels) at the working size and at the full size.  Values are written with
repr(), so a part read back and written again gives the same bytes."""
import os

CSV_NAME = "affinity.csv"


def part_name(rank):
    return "affinity.part%d.csv" % rank


def frame_losses(values):
    """float64 [3] or [6] of one frame (FramePipeline.affinity[i]) -> (loss_work,) or (loss_work, loss_full)"""
    v = [float(x) for x in values]
    if len(v) not in (3, 6):
        raise ValueError("a frame has 3 or 6 affinity values, got %d" % len(v))
    return tuple(sum(v[j:j + 3]) for j in range(0, len(v), 3))


def write_csv(path, per_frame):
    """per_frame: {frame index: (loss_work[, loss_full])} -> the file, in frame order"""
    with open(path, "w") as f:
        for i in sorted(per_frame):
            f.write(",".join([str(int(i))] + [repr(float(v)) for v in per_frame[i]]) + "\n")
    return path


def read_csv(path):
    rows = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            cells = line.strip().split(",")
            if len(cells) not in (2, 3):
                raise ValueError("%s line %d: expected index,loss_work[,loss_full], got %r" % (path, n, line.strip()))
            rows[int(cells[0])] = tuple(float(c) for c in cells[1:])
    return rows


def join_parts(parts, out_path, n_frames=None):
    """The shards' parts, in any order, into the one file a single process writes.  A missing part, a frame present twice or
    (with n_frames) a frame missing is an error that names it."""
    rows = {}
    for p in parts:
        if not os.path.exists(p):
            raise FileNotFoundError("affinity part %s is missing" % p)
        for i, v in read_csv(p).items():
            if i in rows:
                raise ValueError("frame %d is in more than one affinity part (%s)" % (i, p))
            rows[i] = v
    if n_frames is not None:
        missing = [i for i in range(n_frames) if i not in rows]
        if missing:
            raise ValueError("no affinity values for frame %d (%d of %d frames missing)" % (missing[0], len(missing), n_frames))
    return write_csv(out_path, rows)


def summary(per_frame):
    """The closing line: mean, max and the frame of the max of the per-frame loss, per size."""
    if not per_frame:
        return "affinity: no frames"
    out = []
    for j, what in enumerate(("working size", "full size")[:len(next(iter(per_frame.values())))]):
        vals = {i: v[j] for i, v in per_frame.items()}
        worst = max(vals, key=vals.get)
        out.append("%s mean %.6e max %.6e (frame %d)" % (what, sum(vals.values()) / len(vals), vals[worst], worst))
    return "affinity (Matting-Laplacian loss, %d frames): %s" % (len(per_frame), "; ".join(out))
