"""Host side of --style_loss (video_transfer.py, image_transfer.py): the weight source, the per-frame file, the join of the
shards' parts and the closing line.  Nothing here touches a GPU.

style.csv has one line per frame, in frame order: ``index,loss_s`` or, under --content_loss, ``index,loss_s,loss_c`` - the
reference's style loss of the written frame against the style image and its content loss against the frame's content
(vstnet_amd/vgg.py).  Values are written with repr(), so a part read back and written again gives the same bytes."""
import os

CSV_NAME = "style.csv"
NAMES = ("loss_s", "loss_c")


def part_name(rank):
    return "style.part%d.csv" % rank


def add_arguments(p):
    """the flags both scripts take"""
    p.add_argument('--style_loss', action='store_true', default=False, help="measure how much of the style survived: the "
                   "reference's VGG-19 style loss (loss_s of models/VGG.py) of every written frame against the style image, on "
                   "the card (an extension; DESIGN.md section 6, \"Style loss\").  Under --styles the style records are those of "
                   "the FIRST style.  Needs --vgg_ckpoint or --synthetic_vgg_weights")
    p.add_argument('--content_loss', action='store_true', default=False, help="--style_loss: also the reference's content loss "
                   "(loss_c: relu4_1 of the written frame against that of its content frame)")
    p.add_argument('--vgg_ckpoint', type=str, default=None, help="--style_loss: the reference's vgg_normalised.pth")
    p.add_argument('--synthetic_vgg_weights', action='store_true', default=False, help="--style_loss: seeded stand-in weights; "
                   "the values then show that the instrument works and nothing more")


def check_args(parser, args, deep_out=False, tiled=False):
    """What the command line alone decides; parser.error (exit status 2) before anything is read or written."""
    if not args.style_loss:
        if args.content_loss:
            parser.error("--content_loss goes with --style_loss")
        if args.vgg_ckpoint or args.synthetic_vgg_weights:
            parser.error("--vgg_ckpoint / --synthetic_vgg_weights go with --style_loss")
        return
    if bool(args.vgg_ckpoint) == bool(args.synthetic_vgg_weights):
        parser.error("--style_loss needs exactly one of --vgg_ckpoint PATH and --synthetic_vgg_weights")
    if deep_out:
        parser.error("--style_loss measures the written 8-bit frame: not with a high-bit-depth output")
    if tiled:
        parser.error("--style_loss measures a whole frame on the card: not with the tiled route")
    if getattr(args, "stub_stylise", False):
        parser.error("--style_loss is measured on the card: not with --stub_stylise")


def load_weights(args):
    """-> what VGGEncoder takes: "synthetic" or the checkpoint's state dict"""
    if args.synthetic_vgg_weights:
        return "synthetic"
    import torch
    return torch.load(args.vgg_ckpoint, map_location="cpu")


def write_csv(path, per_frame):
    """per_frame: {frame index: (loss_s[, loss_c])} -> the file, in frame order"""
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
                raise ValueError("%s line %d: expected index,loss_s[,loss_c], got %r" % (path, n, line.strip()))
            rows[int(cells[0])] = tuple(float(c) for c in cells[1:])
    return rows


def join_parts(parts, out_path, n_frames=None):
    """The shards' parts, in any order, into the one file a single process writes.  A missing part, a frame present twice or
    (with n_frames) a frame missing is an error that names it."""
    rows = {}
    for p in parts:
        if not os.path.exists(p):
            raise FileNotFoundError("style part %s is missing" % p)
        for i, v in read_csv(p).items():
            if i in rows:
                raise ValueError("frame %d is in more than one style part (%s)" % (i, p))
            rows[i] = v
    if n_frames is not None:
        missing = [i for i in range(n_frames) if i not in rows]
        if missing:
            raise ValueError("no style values for frame %d (%d of %d frames missing)" % (missing[0], len(missing), n_frames))
    return write_csv(out_path, rows)


def summary(per_frame):
    """The closing line: mean, max and the frame of the max, per value."""
    if not per_frame:
        return "style loss: no frames"
    out = []
    for j, what in enumerate(NAMES[:len(next(iter(per_frame.values())))]):
        vals = {i: v[j] for i, v in per_frame.items()}
        worst = max(vals, key=vals.get)
        out.append("%s mean %.6e max %.6e (frame %d)" % (what, sum(vals.values()) / len(vals), vals[worst], worst))
    return "style loss (VGG-19 relu1_1..relu4_1, %d frames): %s" % (len(per_frame), "; ".join(out))
