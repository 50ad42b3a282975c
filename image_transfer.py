#!/usr/bin/env python
"""Single-image style transfer — drop-in for the reference's image_transfer.py (same flags and call sequence,
image_transfer.py:15-37,172-221) on the MI355X HIP path; no torchvision / todos / pdb.

    python image_transfer.py --mode photorealistic --ckpoint checkpoints/photo_image.pt \
        --content data/content/01.jpg --style data/style/01.jpg [--alpha_c 0.3] [--content_seg c.png --style_seg s.png]

Style interpolation (the reference's cWCT.interpolation, models/cWCT.py:206-262), also under masks:
    --styles A B ... [--alpha_s a b ...]    mix several styles (weights sum to 1; default: equal)
    --style_segs sa.png sb.png ...          one label map per style (with --content_seg)
    --interpolate_labels                    with masks: apply --alpha_c and --styles per label.  Without it masks + --alpha_c
                                            behave like the reference (alpha_c is ignored; one line on stderr says so).

--auto_seg segments the content and the style image on the device (vstnet_amd/segformer.py: SegFormer MiT-B1..B5, ADE20K labels),
remaps the two maps as the reference does (self_remapping of both, cross_remapping of the content map) and runs the masked
transfer on the device maps.  The remapping needs the relation table --label_mapping (ade20k_semantic_rel.npy, not shipped
here): without the file --auto_seg is an error, unless --no_seg_remap says that the maps are to be used as segmented.  It needs --seg_ckpoint PATH (a SegmentModel state dict) or
--synthetic_seg_weights; --seg_variant b1..b5 picks the backbone (default b4).  The remapped maps are written to
out_dir/segmentation/ (--save_seg_label, --save_seg_color with --palette).  --seg_size S segments a bicubic downscale of each
image (long edge S) and samples the logits at the image's own size ("Working resolution"); with it --auto_seg also
works for images that take the tiled route.
--strength_map FILE blends the stylised code with the content's per pixel: any image file, read as
8-bit grey, white = full stylisation, black = the untouched content.  It is resized to the stylised size (PIL BILINEAR; for
--mode artistic then to the half-size code grid with PIL BOX) and s = v / 255 scales the cWCT of every code pixel,
y = x + s (A(x) - x): the map form of --alpha_c, with which (and with masks, --auto_seg, --styles, --preserve_luminance) it
combines.  Not on the tiled route.
--strength_labels SPEC [--strength_default D] gives the labels of the CONTENT map (--content_seg, or --auto_seg's map before it is
remapped) a strength each: "12:0.2,20:0" keeps label 12 at 0.2 and label 20 untouched, every other label gets D (default 1).
The map is made on the card (cWCT.frame_strength) and multiplies --strength_map's where both are given.  Photorealistic mode.
--style_map FILE (with two --styles) / --style_maps F_0 ... F_{K-1} (with K --styles) paint WHICH style goes where (DESIGN.md
section 5, "Style maps"): grey images read and resized like --strength_map.  One file is the weight of the second style (black =
the first style, white = the second: t = v / 255, w = (1 - t, t)); K files give w_k = v_k / sum_j v_j per pixel (a pixel whose
planes are all 0 is an error).  The result is sum_k w_k(p) A_k(x) per code pixel, the map form of --alpha_s, which it replaces
(with --alpha_s_end); it combines with --alpha_c, --strength_map and --preserve_luminance, not with masks, --auto_seg or the
tiled route.
--upscale guided [--upscale_radius R] [--upscale_eps E] writes the result at the SOURCE image's size instead of the resized one
(an extension; DESIGN.md section 6, "Guided upscale"): the stylised image is fitted as a locally affine function of the resized
content and the coefficients are applied to the source image on the card.  R = 4 and E = 1e-3 are starting values: picture
quality has not been measured.  Photorealistic mode; an error on the tiled route; an image that is not resized has nothing to
upscale (one stderr line, the plain result).
--affinity [--affinity_map FILE] [--affinity_radius R] [--affinity_eps E] prints the result's Matting-Laplacian loss against the
content image (an extension; DESIGN.md section 6, "Affinity loss"; vstnet_amd/matting.py): the written uint8 image against the
resized content, or under --upscale guided the float stylised image at the stylised size and the written image against the
source at the full size.  FILE gets a grey heat map of the gradient's norm at the stylised size.  The result does not change;
an error on the tiled route.
--style_loss [--content_loss] (--vgg_ckpoint PATH | --synthetic_vgg_weights) prints the written image's VGG-19 style loss against
the style image (the reference's loss_s; under --styles the style records are those of the first style) and, with --content_loss,
its content loss against the content (loss_c), both on the card (vstnet_amd/vgg.py; DESIGN.md section 6, "Style loss").  On
synthetic weights the values show that the instrument works and nothing more.  An error on the tiled route.
--synthetic_weights runs with the deterministic synthetic checkpoint (no trained checkpoint ships with the repo).
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

from utils.utils import img_resize, load_segment, style_map_weights, to_tensor_u8


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', type=str, default='photorealistic')
    p.add_argument('--ckpoint', type=str, default='checkpoints/photo_image.pt')
    p.add_argument('--content', type=str, default='data/content/01.jpg')
    p.add_argument('--style', type=str, default='data/style/01.jpg')
    p.add_argument('--out_dir', type=str, default="output")
    p.add_argument('--max_size', type=int, default=1280)
    p.add_argument('--alpha_c', type=float, default=None)
    p.add_argument('--content_seg', type=str, default=None)
    p.add_argument('--style_seg', type=str, default=None)
    p.add_argument('--auto_seg', action='store_true', default=False)
    p.add_argument('--synthetic_weights', action='store_true', default=False)
    p.add_argument('--precision', type=str, default=None, help="conv arithmetic (default: the library's, bf16x3)")
    # the delldu fork's post-process (project/image_style/vstnet.py:189-220): keep the content's Lab luminance
    p.add_argument('--preserve_luminance', action='store_true', default=False)
    p.add_argument('--label_mapping', type=str, default='models/segmentation/ade20k_semantic_rel.npy')
    p.add_argument('--min_ratio', type=float, default=0.01)
    p.add_argument('--upscale', type=str, default='bicubic', choices=('bicubic', 'guided'), help="guided: write the result at the "
                   "source image's size - a colour guided filter fitted at the stylised size carries the stylisation over to "
                   "the source image on the card (vstnet_amd/guided.py); bicubic (default): the result has the stylised size, "
                   "as always.  Photorealistic mode, not on the tiled route")
    p.add_argument('--affinity', action='store_true', default=False, help="print the result's Matting-Laplacian loss against the "
                   "content image, measured on the card (DESIGN.md section 6, \"Affinity loss\"); the result does not change.  "
                   "Not on the tiled route")
    from vstnet_amd import style_files
    style_files.add_arguments(p)
    p.add_argument('--affinity_map', type=str, default=None, help="--affinity: write an 8-bit grey heat map here, per pixel the norm "
                   "over the channels of the loss's gradient at the stylised size, scaled so that its maximum is 255")
    p.add_argument('--affinity_radius', type=int, default=1, help="--affinity: the window radius, 1..3 (the reference's win_rad)")
    p.add_argument('--affinity_eps', type=float, default=1e-7, help="--affinity: the ridge (the reference's eps), > 0")
    p.add_argument('--upscale_radius', type=int, default=4, help="--upscale guided: the window radius at the stylised size, 1..8")
    p.add_argument('--upscale_eps', type=float, default=1e-3, help="--upscale guided: the ridge on the guide's covariance, > 0")
    add_seg_arguments(p)
    add_mix_arguments(p)
    add_strength_argument(p)
    add_style_map_arguments(p)
    return p


MAX_STYLES = 8


def add_style_map_arguments(p):
    """--style_map / --style_maps, shared with video_transfer.py."""
    p.add_argument('--style_map', type=str, default=None, metavar='FILE',
                   help="with two --styles: a grey-scale image (read as 8-bit grey), per pixel the weight of the SECOND style: "
                        "black = the first style, white = the second; resized like --strength_map")
    p.add_argument('--style_maps', type=str, nargs='+', default=None, metavar='FILE',
                   help="with K --styles: one grey-scale image per style; per pixel the styles are mixed by v_k / sum_j v_j")


def check_style_map_args(parser, args):
    """--style_map / --style_maps, checked before any GPU work and before check_mix_args fills the defaults in: argparse errors
    (exit status 2, usage on stderr).  Returns the list of map files, or None without the flags."""
    if args.style_map is None and args.style_maps is None:
        return None
    if args.style_map is not None and args.style_maps is not None:
        parser.error("--style_map (one file, two styles) and --style_maps (one file per style) are mutually exclusive")
    files = [args.style_map] if args.style_map is not None else list(args.style_maps)
    flag = "--style_map" if args.style_map is not None else "--style_maps"
    n = len(args.styles) if args.styles is not None else 1
    if args.style_map is not None and n != 2:
        parser.error("--style_map is the weight of the second of two styles: it needs --styles A B (got %d style%s); "
                     "--style_maps takes one map per style" % (n, "" if n == 1 else "s"))
    if args.style_maps is not None and (len(files) != n or not 2 <= n <= MAX_STYLES):
        parser.error("--style_maps takes one map per style for 2..%d --styles: %d maps for %d style%s"
                     % (MAX_STYLES, len(files), n, "" if n == 1 else "s"))
    if args.alpha_s is not None or getattr(args, "alpha_s_end", None) is not None:
        parser.error("%s takes the place of the styles' weights: it excludes --alpha_s%s"
                     % (flag, " / --alpha_s_end" if hasattr(args, "alpha_s_end") else ""))
    masks = [f for f in ("content_seg", "content_seg_dir", "style_seg", "style_segs") if getattr(args, f, None) is not None]
    masks += [f for f in ("auto_seg", "interpolate_labels", "seg_remap") if getattr(args, f, False)]
    if masks or args.strength_labels is not None:
        parser.error("%s: style maps are not supported on the masked routes (it excludes --%s)"
                     % (flag, (masks + ["strength_labels"])[0]))
    for f in files:
        if not os.path.isfile(f):
            parser.error("%s %s: no such file" % (flag, f))
    return files


def check_style_map_planes(parser, args, files, size_wh, sizes_wh=()):
    """The rest of the checks, still before any GPU work: sizes_wh = stylised sizes of images that must not need the tiled
    route; size_wh = the stylised size of the content, at which the planes are loaded to look for a pixel that no plane covers."""
    flag = "--style_map" if args.style_map is not None else "--style_maps"
    from vstnet_amd import tiled
    for w, h in sizes_wh:
        if tiled.needs_tiling(h, w, float("inf")):
            parser.error("%s does not work on the tiled route, which a %dx%d image takes: lower --max_size" % (flag, w, h))
    try:
        load_style_map(files, size_wh, args.mode)
    except ValueError as e:
        parser.error("%s: %s" % (flag, e))


def load_style_map(paths, size_wh, mode):
    """The weight planes of --style_map / --style_maps for frames stylised at size_wh: every file read and resized exactly as
    load_strength_map does (8-bit grey, BILINEAR to the stylised size, for artistic codes then BOX to the half-size code grid),
    then utils.style_map_weights on the 8-bit planes: float32 [K, cH, cW] at the code's resolution.  A pixel that no plane
    covers raises ValueError, which names it."""
    w, h = size_wh
    planes = []
    for path in paths:
        img = Image.fromarray(load_matte(path, size_wh))
        if mode.lower() == "artistic":
            img = img.resize((w // 2, h // 2), Image.BOX)
        planes.append(np.asarray(img, dtype=np.uint8))
    return style_map_weights(planes)


def add_strength_argument(p):
    """--strength_map, shared with video_transfer.py."""
    p.add_argument('--strength_map', type=str, default=None, metavar='FILE',
                   help="a grey-scale image (any format; read as 8-bit grey): per pixel, white = full stylisation, black = the "
                        "untouched content; resized to the stylised size, one map for the image / for every frame of a clip")
    p.add_argument('--strength_labels', type=str, default=None, metavar='SPEC',
                   help="a strength per label of the content's label map (--content_seg, --content_seg_dir, --auto_seg before "
                        "remapping): LABEL:STRENGTH[,LABEL:STRENGTH...], e.g. 12:0.2,20:0; multiplies --strength_map / --strength_dir")
    p.add_argument('--strength_default', type=float, default=1.0, metavar='D',
                   help="--strength_labels: the strength of every label the list does not name (default 1)")


def check_strength_args(parser, args, sizes_wh=()):
    """--strength_map, checked before any GPU work: argparse errors (exit status 2, usage on stderr).  sizes_wh: the stylised
    sizes of images that must not need the tiled route (it has no strength maps)."""
    if args.strength_labels is not None:
        from vstnet_amd.cwct import cWCT
        has_labels = args.auto_seg or args.content_seg is not None or getattr(args, "content_seg_dir", None) is not None
        if not has_labels:
            parser.error("--strength_labels names labels of the content's map: it needs --content_seg%s or --auto_seg"
                         % (" / --content_seg_dir" if hasattr(args, "content_seg_dir") else ""))
        if args.mode.lower() != "photorealistic":
            parser.error("--strength_labels needs --mode photorealistic (label maps have the frame's resolution)")
        try:
            cWCT.strength_table(args.strength_labels, args.strength_default)
        except ValueError as e:
            parser.error("--strength_labels / --strength_default: %s" % e)
    elif args.strength_default != 1.0:
        parser.error("--strength_default belongs to --strength_labels")
    if args.strength_map is not None and not os.path.isfile(args.strength_map):
        parser.error("--strength_map %s: no such file" % args.strength_map)
    from vstnet_amd import tiled
    for w, h in sizes_wh:
        if tiled.needs_tiling(h, w, float("inf")):
            parser.error("--strength_map / --strength_labels do not work on the tiled route, which a %dx%d image takes: lower "
                         "--max_size" % (w, h))


def load_strength_map(path, size_wh, mode):
    """The map of --strength_map for frames stylised at size_wh: 8-bit grey, BILINEAR to the stylised size, for artistic codes
    then BOX to the half-size code grid; float32 [cH, cW] = v / 255 at the code's resolution."""
    w, h = size_wh
    img = Image.fromarray(load_matte(path, size_wh))
    if mode.lower() == "artistic":
        img = img.resize((w // 2, h // 2), Image.BOX)
    return np.asarray(img, dtype=np.float32) / np.float32(255.0)


def load_matte(path, size_wh=None):
    """A grey map file as 8-bit grey, uint8 [H,W]; with size_wh PIL-BILINEAR-resized to it (the stylised size)."""
    img = Image.open(path).convert("L")
    if size_wh is not None and img.size != tuple(size_wh):
        img = img.resize(tuple(size_wh), Image.BILINEAR)
    return np.array(img, dtype=np.uint8)            # (a copy: writable, so that torch takes it without a warning)


def add_seg_arguments(p):
    """--auto_seg's companions, shared with video_transfer.py."""
    p.add_argument('--seg_ckpoint', type=str, default=None, help="--auto_seg: a SegmentModel state dict (backbone.* / decode_head.*)")
    p.add_argument('--synthetic_seg_weights', action='store_true', default=False,
                   help="--auto_seg: the deterministic synthetic segmenter weights (no trained segmenter ships with the repo)")
    p.add_argument('--seg_variant', type=str, default='b4', choices=('b1', 'b2', 'b3', 'b4', 'b5'))
    p.add_argument('--no_seg_remap', action='store_true', default=False,
                   help="--auto_seg: use the maps as segmented, without self_/cross_remapping (no relation table needed)")
    p.add_argument('--seg_size', type=int, default=None, metavar='S',
                   help="--auto_seg: segment a bicubic downscale of each image / frame whose long edge is S (>= 32) and sample "
                        "the logits at the full size; without it the segmenter runs at the stylised resolution")
    p.add_argument('--save_seg_label', action='store_true', default=True)
    p.add_argument('--save_seg_color', action='store_true', default=True)
    p.add_argument('--palette', type=str, default='models/segmentation/ade20k_palette.npy')


def check_seg_args(parser, args):
    """--auto_seg's arguments, checked before any GPU work: argparse errors (exit status 2, usage on stderr)."""
    if not args.auto_seg:
        if args.seg_ckpoint is not None or args.synthetic_seg_weights:
            parser.error("--seg_ckpoint / --synthetic_seg_weights belong to --auto_seg")
        if args.seg_size is not None:
            parser.error("--seg_size belongs to --auto_seg")
        return
    if args.seg_size is not None and args.seg_size < 32:
        parser.error("--seg_size must be at least 32 (the segmenter's smallest frame edge)")
    if args.seg_ckpoint is None and not args.synthetic_seg_weights:
        parser.error("--auto_seg needs the segmenter's weights: --seg_ckpoint PATH or --synthetic_seg_weights")
    if args.seg_ckpoint is not None and args.synthetic_seg_weights:
        parser.error("--seg_ckpoint and --synthetic_seg_weights are mutually exclusive")
    if getattr(args, "content_seg_dir", None) is not None:
        parser.error("--auto_seg makes every frame's map itself: it excludes --content_seg_dir")
    if args.content_seg is not None or args.style_seg is not None or args.style_segs is not None:
        parser.error("--auto_seg makes the label maps itself: it excludes --content_seg / --style_seg / --style_segs")
    if args.styles is not None and len(args.styles) > 1:
        parser.error("--auto_seg takes one style (--styles with several images is not supported with it)")
    if args.interpolate_labels:
        parser.error("--auto_seg does not combine with --interpolate_labels")
    if getattr(args, "alpha_s_end", None) is not None:
        parser.error("--auto_seg does not combine with --alpha_s_end")
    if hasattr(args, "video") and args.mode.lower() != "photorealistic":
        parser.error("--auto_seg on video needs --mode photorealistic (masked artistic codes have no per-frame route)")
    if not args.no_seg_remap and not os.path.exists(args.label_mapping):
        parser.error("--auto_seg remaps its label maps with the relation table, and --label_mapping %s is not there; "
                     "--no_seg_remap uses the maps as segmented" % args.label_mapping)
    if getattr(args, "stub_stylise", False):
        parser.error("--auto_seg runs on the GPU: it excludes --stub_stylise")


def build_segmenter(args, device):
    """The device SegFormer of --auto_seg with its weights loaded."""
    from vstnet_amd.segformer import SegFormer
    from vstnet_amd.synth import SEG_DEPTHS, synthetic_segformer_state_dict
    dim = 256 if args.seg_variant == 'b1' else 768           # (SegFormerHead: embedding_dim 256 for B1)
    seg = SegFormer(args.seg_variant, embedding_dim=dim, device=device)
    if args.synthetic_seg_weights:
        sd = synthetic_segformer_state_dict(4321, SEG_DEPTHS[args.seg_variant], dim)
    else:
        sd = torch.load(args.seg_ckpoint, map_location="cpu", weights_only=True)
        sd = sd['state_dict'] if 'state_dict' in sd else sd
    return seg.load_state_dict(sd)


def device_remapper(args):
    """DeviceSegReMapping over --label_mapping, or None with --no_seg_remap (check_seg_args has seen to the file)."""
    if args.no_seg_remap:
        return None
    from vstnet_amd.masks import DeviceSegReMapping
    return DeviceSegReMapping(args.label_mapping, args.min_ratio)


def save_seg_maps(args, maps, out_dir, quiet=False):
    """maps: {file stem: uint8 [H,W] labels}.  image_transfer.py:134-152 of the reference: <stem>_label.png, <stem>_color.png."""
    import sys
    seg_dir = os.path.join(out_dir, "segmentation")
    palette = None
    if args.save_seg_color:
        if os.path.exists(args.palette):
            palette = np.load(args.palette).astype(np.uint8)
        elif not quiet:
            print("--save_seg_color: the palette %s is missing, no coloured maps are written" % args.palette, file=sys.stderr)
    if not (args.save_seg_label or palette is not None):
        return
    os.makedirs(seg_dir, exist_ok=True)
    for stem, m in maps.items():
        if args.save_seg_label:
            Image.fromarray(m).save(os.path.join(seg_dir, stem + "_label.png"))
        if palette is not None:
            lut = np.zeros((256, 3), np.uint8)
            lut[:len(palette)] = palette[:256]
            Image.fromarray(lut[m]).save(os.path.join(seg_dir, stem + "_color.png"))


def check_seg_pixels(seg_size, sizes_wh):
    """--auto_seg's size limits for images / frames of ``sizes_wh``, before any of them is segmented: the network runs on at most
    MAX_PIXELS pixels (the working size under --seg_size), a label map holds at most MAX_LABEL_PIXELS."""
    from vstnet_amd.segformer import MAX_LABEL_PIXELS, MAX_PIXELS, SegFormer
    for w, h in sizes_wh:
        hw, ww = SegFormer.work_hw(h, w, seg_size)
        if hw * ww > MAX_PIXELS and seg_size is None:
            raise SystemExit("--auto_seg segments whole frames of at most %d pixels (there is no tiled segmentation); %dx%d is "
                             "larger: pass --seg_size S to segment a downscaled copy, or lower --max_size" % (MAX_PIXELS, w, h))
        if hw * ww > MAX_PIXELS:
            raise SystemExit("--seg_size %d segments a %dx%d frame at %dx%d, more than %d pixels: lower --seg_size"
                             % (seg_size, w, h, ww, hw, MAX_PIXELS))
        if w * h > MAX_LABEL_PIXELS:
            raise SystemExit("--auto_seg makes label maps of at most %d pixels; %dx%d is larger: lower --max_size"
                             % (MAX_LABEL_PIXELS, w, h))


def segment_image(segmenter, img, seg_size, device, host_resize=False):
    """One PIL image -> its uint8 [H,W] device label map.  With --seg_size the working copy is made on the card from the
    uploaded image, or (host_resize: the image is too large to stylise whole, so it is not uploaded whole either) by PIL on the
    host - the same bytes, so the same map."""
    if seg_size is None:
        return segmenter.segment_u8(to_tensor_u8(img)[0].to(device))
    if not host_resize:
        return segmenter.segment_u8(to_tensor_u8(img)[0].to(device), work_size=seg_size)
    w, h = img.size
    hw, ww = segmenter.work_hw(h, w, seg_size)
    work = img if (hw, ww) == (h, w) else img.resize((ww, hw), Image.BICUBIC)
    return segmenter.segment_work_u8(to_tensor_u8(work)[0].to(device), (h, w))


def auto_segment(args, segmenter, content_img, style_img, device, host_resize=False, raw=None):
    """The reference's --auto_seg branch (image_transfer.py:75-155) on the device: segment both images, self_remapping of both,
    cross_remapping of the content map.  Returns the two remapped maps as uint8 [H,W] device tensors.  raw (a list): the content
    map as segmented, before any remapping, is appended to it."""
    with torch.no_grad():
        c = segment_image(segmenter, content_img, args.seg_size, device, host_resize)
        if raw is not None:
            raw.append(c.clone())
        s = segment_image(segmenter, style_img, args.seg_size, device, host_resize)
        remap = device_remapper(args)
        if remap is not None:
            c, s = remap.self_remapping(c), remap.self_remapping(s)
            c = remap.cross_remapping(c, s)
            remap.check()
    return c, s


def add_mix_arguments(p):
    """Style interpolation flags shared with video_transfer.py (all additive)."""
    p.add_argument('--styles', type=str, nargs='+', default=None, help="several style images to mix (instead of --style)")
    p.add_argument('--alpha_s', type=float, nargs='+', default=None, help="one weight per style, summing to 1 (default: equal)")
    p.add_argument('--style_segs', type=str, nargs='+', default=None, help="one label map per style of --styles")
    p.add_argument('--interpolate_labels', action='store_true', default=False,
                   help="with masks: apply --alpha_c and --styles per label (the reference ignores alpha_c under masks)")


def _check_weights(w, n, flag):
    if len(w) != n:
        raise SystemExit("%s: %d weights for %d styles" % (flag, len(w), n))
    if any(a < 0.0 for a in w) or abs(sum(w) - 1.0) > 1e-6:
        raise SystemExit("%s must be non-negative and sum to 1 (got %s, sum %.9g)" % (flag, w, sum(w)))


def check_mix_args(args, err=None):
    """Checks --styles / --alpha_s / --style_segs / --interpolate_labels (and --alpha_s_end of video_transfer.py) before any GPU
    work and fills args.styles, args.alpha_s, args.style_segs (None without masks).  Returns True when the masked path
    interpolates per label."""
    import sys
    err = err or sys.stderr
    if args.styles is None:
        args.styles = [args.style]
    else:
        args.style = args.styles[0]          # (output names keep following --style)
    n = len(args.styles)
    if not 1 <= n <= MAX_STYLES:
        raise SystemExit("--styles takes 1..%d images, got %d" % (MAX_STYLES, n))
    if args.alpha_s is None:
        args.alpha_s = [1.0 / n] * n
    _check_weights(args.alpha_s, n, "--alpha_s")
    if getattr(args, "alpha_s_end", None) is not None:
        _check_weights(args.alpha_s_end, n, "--alpha_s_end")
    if args.alpha_c is not None and not 0.0 <= args.alpha_c <= 1.0:
        raise SystemExit("--alpha_c must be in [0, 1]")
    if args.style_segs is None and args.style_seg is not None:
        args.style_segs = [args.style_seg] if n == 1 else None
    if args.style_segs is not None and len(args.style_segs) != n:
        raise SystemExit("--style_segs: %d maps for %d styles" % (len(args.style_segs), n))
    has_cseg = args.content_seg is not None or getattr(args, "content_seg_dir", None) is not None
    masked = has_cseg and args.style_segs is not None
    if has_cseg and n > 1 and args.style_segs is None:
        raise SystemExit("masks with several styles need --style_segs (one map per style)")
    if masked and n > 1 and not args.interpolate_labels:
        raise SystemExit("several styles under masks need --interpolate_labels")
    world = int(str(getattr(args, "shard", "0/1")).split("/")[1])
    said_by_parent = world > 1 and getattr(args, "gpus", 1) == 1      # a child of --gpus N: the parent has said it
    if masked and args.alpha_c is not None and not args.interpolate_labels and not said_by_parent:
        print("alpha_c is ignored with masks (the reference's behaviour); pass --interpolate_labels to apply it per label",
              file=err)
    if masked:
        args.style_seg = args.style_segs[0]
    return bool(masked and args.interpolate_labels)


def build_network(mode, ckpoint, synthetic, device, precision=None):
    from models.RevResNet import RevResNet
    if mode.lower() == "photorealistic":
        hd, sp = 16, 2
    elif mode.lower() == "artistic":
        hd, sp = 64, 1
    else:
        raise NotImplementedError()
    net = RevResNet(hidden_dim=hd, sp_steps=sp, precision=precision)
    if synthetic:
        from vstnet_amd.synth import synthetic_state_dict
        net.load_state_dict(synthetic_state_dict(1234, hd, sp))
    else:
        state_dict = torch.load(ckpoint, map_location="cpu", weights_only=True)
        net.load_state_dict(state_dict['state_dict'])
    return net.to(device).eval()


def stylize(net, cwct, content_img, style_img, content_seg=None, style_seg=None, alpha_c=None, device="cuda",
            preserve_luminance=False, alpha_s=None, interpolate_labels=False, strength=None, style_map=None, upscale=None,
            affinity=None):
    """image_transfer.py:172-201 with the uint8 frame edge on the device; returns uint8 [H,W,3] numpy.  style_img / style_seg
    may be lists (several styles, weights alpha_s); interpolate_labels applies alpha_c and the mix per label under masks.
    strength: a float map in [0, 1] at the code's resolution (load_strength_map), a bound map (cWCT.frame_strength), or None.
    style_map: float [K, cH, cW] weight planes (load_style_map) or a bound map (cWCT.bind_style_map) for the K styles, in place
    of alpha_s; not with masks.
    upscale: (source image as a uint8 [H,W,3] array, radius, eps): the result is the guided upscale of the stylised image to
    the source's size (vstnet_amd/guided.py), behind the Lab step of preserve_luminance.
    affinity: a dict with "radius" and "eps"; with `upscale` it gets "work" = (loss3, gradient) of the float stylised image
    against the content at the stylised size (vstnet_amd/matting.py) - the image main() cannot see.  Nothing else changes."""
    styles = list(style_img) if isinstance(style_img, (list, tuple)) else [style_img]
    segs = None if style_seg is None else (list(style_seg) if isinstance(style_seg, (list, tuple)) else [style_seg])
    masked = content_seg is not None and segs is not None
    if len(styles) > 1 and masked and not interpolate_labels:
        raise ValueError("several styles under masks need interpolate_labels=True")
    with torch.no_grad():
        z_c = net.forward_u8(to_tensor_u8(content_img).to(device))
        z_ss = [net.forward_u8(to_tensor_u8(im).to(device)) for im in styles]
        if style_map is not None:
            if masked:
                raise ValueError("style maps are not supported on the masked routes")
            z_cs = cwct.interpolation(z_c, z_ss, None, 0.0 if alpha_c is None else alpha_c, strength=strength, style_map=style_map)
        elif len(styles) > 1 or (masked and interpolate_labels):
            w = [1.0 / len(styles)] * len(styles) if alpha_s is None else list(alpha_s)
            z_cs = cwct.interpolation(z_c, z_ss, w, 0.0 if alpha_c is None else alpha_c, content_seg if masked else None,
                                      segs if masked else None, strength=strength)
        elif alpha_c is not None and content_seg is None and style_seg is None:
            assert 0.0 <= alpha_c <= 1.0
            z_cs = cwct.interpolation(z_c, styl_feat_list=[z_ss[0]], alpha_s_list=[1.0], alpha_c=alpha_c, strength=strength)
        else:
            z_cs = cwct.transfer(z_c, z_ss[0], content_seg, None if segs is None else segs[0], strength=strength)
        if upscale is not None:
            from vstnet_amd.guided import guided_apply, guided_fit
            src, radius, eps = upscale
            content_u8 = to_tensor_u8(content_img).to(device)
            sty = net(z_cs, forward=False)
            if preserve_luminance:
                from vstnet_amd.color import luminance_transfer_u8
                sty = luminance_transfer_u8(content_u8, sty, out=sty, to_float=True)
            if affinity is not None:
                from vstnet_amd.matting import matting_loss
                affinity["work"] = matting_loss(content_u8, sty, affinity["radius"], affinity["eps"], grad=True)
            coef = guided_fit(content_u8, sty, radius, eps)
            return guided_apply(coef, torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8)).to(device))[0].cpu().numpy()
        if not preserve_luminance:
            return net.inverse_u8(z_cs)[0].cpu().numpy()
        from vstnet_amd.color import luminance_transfer
        content = to_tensor_u8(content_img).to(device).permute(0, 3, 1, 2).float().div(255.0)
        out = luminance_transfer(content, net(z_cs, forward=False))
        return out[0].mul(255.0).clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy()


def check_upscale_args(parser, args):
    """--upscale guided, before any GPU work: the flags, the mode, the tiled route (as far as the whole-frame guard decides it)
    and an image that is not resized at all - nothing to upscale: one stderr line, and the plain path is in force."""
    import sys
    if args.upscale != 'guided':
        return
    if not 1 <= args.upscale_radius <= 8:
        parser.error("--upscale_radius must be in 1..8")
    if not 0.0 < args.upscale_eps < float("inf"):
        parser.error("--upscale_eps must be above 0 (and finite)")
    if args.mode != 'photorealistic':
        parser.error("--upscale guided fits the stylised image as a locally affine function of the content, which the "
                     "photorealistic model is trained to be and the artistic one is not: not with --mode %s" % args.mode)
    from vstnet_amd import tiled
    from vstnet_amd.resize import img_resize_size
    size = Image.open(args.content).size
    w, h = img_resize_size(size, args.max_size, 4)
    if tiled.needs_tiling(h, w, float("inf")):
        parser.error("--upscale guided does not work on the tiled route, which a %dx%d image takes: lower --max_size" % (w, h))
    if (w, h) == tuple(size):
        print("--upscale guided: a %dx%d image is stylised at its own size, there is nothing to upscale: the plain path is in "
              "force" % (w, h), file=sys.stderr)
        args.upscale = 'bicubic'


def check_affinity_args(parser, args):
    """--affinity, before any GPU work: the flags, and the tiled route as far as the whole-frame guard decides it"""
    if not args.affinity:
        if args.affinity_map is not None:
            parser.error("--affinity_map belongs to --affinity")
        return
    if not 1 <= args.affinity_radius <= 3:
        parser.error("--affinity_radius must be in 1..3")
    if not 0.0 < args.affinity_eps < float("inf"):
        parser.error("--affinity_eps must be above 0 (and finite)")
    from vstnet_amd import tiled
    from vstnet_amd.resize import img_resize_size
    w, h = img_resize_size(Image.open(args.content).size, args.max_size, 4)
    if tiled.needs_tiling(h, w, float("inf")):
        parser.error("--affinity does not work on the tiled route, which a %dx%d image takes: lower --max_size" % (w, h))


def check_style_loss_args(parser, args):
    """--style_loss, before any GPU work: the flags first (nothing is read for those), then the tiled route as far as the
    whole-frame guard decides it"""
    from vstnet_amd import style_files
    style_files.check_args(parser, args)
    if not args.style_loss:
        return
    if args.content_loss and args.upscale == 'guided':
        parser.error("--content_loss compares the written image with the content at the stylised size: not with --upscale guided")
    from vstnet_amd import tiled
    from vstnet_amd.resize import img_resize_size
    w, h = img_resize_size(Image.open(args.content).size, args.max_size, 4)
    style_files.check_args(parser, args, tiled=tiled.needs_tiling(h, w, float("inf")))
    if min(w, h) < 9 or min(img_resize_size(Image.open((args.styles or [args.style])[0]).size, args.max_size, 4)) < 9:
        parser.error("--style_loss needs a content and a style of at least 9x9 after the resize")


def report_style_loss(args, content, style, out, device):
    """--style_loss: loss_s of the written image `out` (uint8 [H,W,3]) against the (first) style image and, with
    --content_loss, loss_c against the content, printed"""
    from vstnet_amd import style_files
    from vstnet_amd.vgg import StyleLoss, VGGEncoder
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(device)      # noqa: E731
    meter = StyleLoss(VGGEncoder(style_files.load_weights(args), device), dev(np.array(style)))
    got = meter(dev(out), dev(np.array(content)) if args.content_loss else None).cpu().numpy()
    values = dict(zip(style_files.NAMES, (float(v) for v in got)))
    print("style loss (VGG-19 relu1_1..relu4_1, written image %dx%d against the style%s): %s"
          % (out.shape[1], out.shape[0], " and the content" if args.content_loss else "",
             ", ".join("%s %.6e" % kv for kv in values.items())))
    return values


def report_affinity(args, content, out, source, measure, device):
    """--affinity: the loss of the result `out` (uint8 [H,W,3]) against the content - at the stylised size, and under --upscale
    guided (source: the full-size image) at both -, printed; --affinity_map from the stylised size's gradient, on the host."""
    from vstnet_amd.matting import matting_loss
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(device)      # noqa: E731
    r, eps = measure["radius"], measure["eps"]
    values = {}
    if source is None:      # the written image is the stylised one: the uint8 form
        loss3, grad = matting_loss(dev(np.array(content)), dev(out), r, eps, grad=True)
        print("affinity (Matting-Laplacian loss, written image against the content, %dx%d): %.6e"
              % (content.size[0], content.size[1], float(loss3.sum())))
    else:
        loss3, grad = measure["work"]
        full = matting_loss(dev(source), dev(out), r, eps)
        values["full"] = float(full.sum())
        print("affinity (Matting-Laplacian loss): stylised size %dx%d (float image) %.6e, full size %dx%d (written image against "
              "the source) %.6e" % (content.size[0], content.size[1], float(loss3.sum()), source.shape[1], source.shape[0],
                                    values["full"]))
    values["work"] = float(loss3.sum())
    if args.affinity_map is not None:
        g = np.sqrt((grad.cpu().numpy().astype(np.float64) ** 2).sum(0))
        top = float(g.max())
        heat = np.zeros(g.shape, np.uint8) if top == 0.0 else np.clip(np.rint(g * (255.0 / top)), 0, 255).astype(np.uint8)
        Image.fromarray(heat).save(args.affinity_map)
        print("Save affinity map at %s" % args.affinity_map)
    return values


LAST_RUN = {}        # what the last main() of this process measured: {"affinity": {"work": loss[, "full": loss]}}


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_affinity_args(parser, args)       # (before any GPU work)
    check_style_loss_args(parser, args)
    check_seg_args(parser, args)
    map_files = check_style_map_args(parser, args)      # (the flags and the files; before check_mix_args fills --alpha_s in)
    per_label = check_mix_args(args)
    check_strength_args(parser, args)       # (the file)
    if map_files is not None:
        # before any GPU work too: the tiled route, and a pixel that no plane covers (the planes at the stylised size)
        from vstnet_amd.resize import img_resize_size
        sizes = [img_resize_size(Image.open(f).size, args.max_size, 4) for f in [args.content] + list(args.styles)]
        check_style_map_planes(parser, args, map_files, sizes[0], sizes)
    if args.strength_map is not None or args.strength_labels is not None:
        # before any GPU work too: sizes that the whole-frame guard sends to the tiled route
        from vstnet_amd.resize import img_resize_size
        check_strength_args(parser, args, [img_resize_size(Image.open(f).size, args.max_size, 4)      # (both nets: down_scale 4)
                                           for f in [args.content] + list(args.styles)])
    check_upscale_args(parser, args)        # (before any GPU work too)
    device = torch.device("cuda")
    os.makedirs(args.out_dir, exist_ok=True)
    net = build_network(args.mode, args.ckpoint, args.synthetic_weights, device, args.precision)
    from models.cWCT import cWCT
    cwct = cWCT(precision=args.precision)

    content = Image.open(args.content).convert('RGB')
    upscale = (np.array(content, dtype=np.uint8), args.upscale_radius, args.upscale_eps) if args.upscale == 'guided' else None
    content = img_resize(content, args.max_size, down_scale=net.down_scale)
    styles = [img_resize(Image.open(f).convert('RGB'), args.max_size, down_scale=net.down_scale) for f in args.styles]
    style = styles[0]
    content_seg = style_seg = style_segs = None
    if args.content_seg is not None and args.style_segs is not None:
        content_seg = load_segment(args.content_seg, content.size)[None, ...]
        style_segs = [load_segment(f, im.size)[None, ...] for f, im in zip(args.style_segs, styles)]
        style_seg = style_segs[0]
    from vstnet_amd import tiled
    budget = tiled.memory_budget(device)
    tiled_route = any(tiled.needs_tiling(im.size[1], im.size[0], budget) for im in [content] + styles)
    if args.auto_seg:
        check_seg_pixels(args.seg_size, [content.size, style.size])
        # (an image on the tiled route is not uploaded whole: with --seg_size its working copy is made by PIL on the host)
        raw_maps = []
        c_map, s_map = auto_segment(args, build_segmenter(args, device), content, style, device,
                                    host_resize=tiled_route and args.seg_size is not None, raw=raw_maps)
        save_seg_maps(args, {"content_seg": c_map.cpu().numpy(), "style_seg": s_map.cpu().numpy()}, args.out_dir)
        # the masked transfer plans its labels from the device maps (cWCT.plan_masks takes uint8 device tensors)
        content_seg, style_seg = c_map[None], s_map[None]
        style_segs = [style_seg]

    strength = None
    if args.strength_map is not None or args.strength_labels is not None:
        if tiled_route:                     # (the device-memory budget sends it there: known only now)
            raise SystemExit("--strength_map / --strength_labels do not work on the tiled route, which this image takes on this "
                             "device: lower --max_size")
    if args.strength_labels is not None:
        # the content's own labels (before --auto_seg's remapping) through the table, times the map if there is one: made on
        # the card, the call a video frame makes per frame
        labels = raw_maps[0] if args.auto_seg else torch.from_numpy(np.ascontiguousarray(
            content_seg[0] if content_seg is not None else load_segment(args.content_seg, content.size))).to(device)
        matte = None if args.strength_map is None else torch.from_numpy(load_matte(args.strength_map, content.size)).to(device)
        w_, h_ = content.size
        strength = cwct.frame_strength((1, 32, h_, w_), matte=matte, labels=labels.contiguous(),
                                       table=cwct.strength_table(args.strength_labels, args.strength_default, device))
    elif args.strength_map is not None:
        strength = load_strength_map(args.strength_map, content.size, args.mode)
    style_map = None
    if map_files is not None:
        if tiled_route:
            raise SystemExit("--style_map / --style_maps do not work on the tiled route, which this image takes on this device: "
                             "lower --max_size")
        style_map = load_style_map(map_files, content.size, args.mode)
    if tiled_route and upscale is not None:         # (the device-memory budget sends it there: known only now)
        raise SystemExit("--upscale guided does not work on the tiled route, which this image takes on this device: lower "
                         "--max_size")
    if tiled_route and args.affinity:
        raise SystemExit("--affinity does not work on the tiled route, which this image takes on this device: lower --max_size")
    if tiled_route and args.style_loss:
        raise SystemExit("--style_loss does not work on the tiled route, which this image takes on this device: lower --max_size")
    measure = dict(radius=args.affinity_radius, eps=args.affinity_eps) if args.affinity else None
    if tiled_route:
        # past the whole-frame guard or the device-memory budget (e.g. --max_size 16384): halo tiles, same result
        if len(styles) > 1:
            raise ValueError("several styles in tiled mode are out of scope: lower --max_size or pass one style")
        host = lambda m: m.cpu().numpy() if torch.is_tensor(m) else m           # noqa: E731  (the tiled driver cuts host maps)
        out = tiled.stylize_tiled(net, cwct, np.array(content, dtype=np.uint8), np.array(style, dtype=np.uint8),
                                  None if content_seg is None else host(content_seg[0]),
                                  None if style_seg is None else host(style_seg[0]),
                                  args.alpha_c, args.preserve_luminance, interpolate_labels=per_label)
    elif len(styles) > 1 or per_label:
        out = stylize(net, cwct, content, styles, content_seg, style_segs, args.alpha_c, device, args.preserve_luminance,
                      alpha_s=args.alpha_s, interpolate_labels=per_label, strength=strength, style_map=style_map, upscale=upscale,
                      affinity=measure)
    else:
        out = stylize(net, cwct, content, style, content_seg, style_seg, args.alpha_c, device, args.preserve_luminance,
                      strength=strength, upscale=upscale, affinity=measure)
    LAST_RUN.clear()
    if measure is not None:
        LAST_RUN["affinity"] = report_affinity(args, content, out, None if upscale is None else upscale[0], measure, device)
    if args.style_loss:
        LAST_RUN["style"] = report_style_loss(args, content, style, out, device)
    cn, sn = os.path.basename(args.content), os.path.basename(args.style)
    path = os.path.join(args.out_dir, "%s_%s.png" % (cn.split(".")[0], sn.split(".")[0]))
    Image.fromarray(out).save(path, quality=100)
    print("Save at %s" % path)
    return path


if __name__ == "__main__":
    main()
