#!/usr/bin/env python
"""Video (frame-sequence) style transfer — drop-in for the reference's video_transfer.py (video_transfer.py:17-38,
160-214) on the MI355X HIP path.

Differences that do not change pixels: the style is encoded and factored ONCE (the reference re-encodes it for
every frame, :195); frames move as uint8 through pinned ring buffers and are quantised on the device; decode/resize,
H2D, compute, D2H and encode overlap (vstnet_amd/pipeline.py) instead of running one after the other.  The writer-size quirk of the
reference is kept (:83-86: video_width is overwritten before it scales video_height, so a 1920x1080 clip at
--max_size 1280 is written at 1280x1080 while frames are stylised at 1280x720).
--video may be a directory of frames (always works) or a video file (needs cv2, optional).  Output: an .mp4 if
cv2 is importable, else numbered PNGs.

Multi-GPU (BASELINE config 5; SURVEY 8(e): frames are independent, the host gathers the outputs):
  --gpus N     this process starts N children BEFORE it touches a GPU — child r gets HIP_VISIBLE_DEVICES=r, a CPU thread cap
               of cores // N and `--shard r/N` —, waits for all of them (a failing child fails the run: non-zero exit, the
               others are terminated, nothing is re-executed) and then merges their outputs into the ONE ordered clip / frame
               directory the reference writes (video_transfer.py:92-96,160-214): every frame index present exactly once.
  --shard i/n  process the i-th contiguous shard of the frames (what the children run; also usable by hand).
Every frame is resized on its own like the reference's loop (:161): a frame whose size differs from its predecessor's gets its
own ring buffers and mask plan instead of an error; the writer size comes from the clip's first frame (:82-86).
--content_seg_dir DIR gives every frame its own label map (the reference segments every frame, :161-186; here the maps come
from files, one per frame, sorted by name): RGB maps in the dictionary colours or single-channel label PNGs.  With --seg_remap
the style map is self-remapped once and every frame's map self- and cross-remapped (the reference's --auto_seg branch).  The
decode workers load and NEAREST-resize the maps; everything after the upload runs on the device (vstnet_amd/masks.py).
Style interpolation (cWCT.interpolation, models/cWCT.py:206-262; the reference's script says "mask is not supported" there,
:198-201): --styles A B ... [--alpha_s a b ...] [--style_segs ...] mixes several styles, --interpolate_labels applies the mix
and --alpha_c per label under masks, --alpha_s_end a b ... cross-fades the weights linearly from the first to the last frame of
the CLIP (a frame's weights depend on its global index only, so shards and --gpus N give the frames one process gives).  The
styles are encoded, reduced and factored once; a frame's mix costs one factor launch.
--resize device moves the two bicubic resizes of every frame (:161) and the resize to the writer size (:210-212) from the host
threads / stock torch ops to HIP kernels on the frame's stream (vstnet_amd/resize.py); the default, host, is unchanged.
--preserve_luminance keeps every frame's own Lab luminance and takes the stylised chroma (image_transfer.py's flag, the delldu
fork's post-process, project/image_style/vstnet.py:189-220): one pointwise HIP launch per frame at the uint8 frame edge
(vstnet_amd/color.py luminance_transfer_u8), at the stylised size and before the resize to the writer size, as image_transfer.py
orders it.  It combines with every route above.

--auto_seg makes the label maps on the card (vstnet_amd/segformer.py: SegFormer MiT-B1..B5; --seg_ckpoint PATH or
--synthetic_seg_weights, --seg_variant b1..b5).  The style image is segmented and self-remapped once per clip; every frame is
segmented on its own stream, from its uint8 device slot (after --resize device, if given) into the mask ring slot that an
uploaded map of --content_seg_dir would fill, and the per-frame mask route takes it from there: self- and cross-remapping as a
256-entry table, the label plan, the redo on the dense route past 8 labels, --shard / --gpus N, --preserve_luminance.  The
remapping needs the relation table --label_mapping; --no_seg_remap uses the maps as segmented.  --save_seg_label /
--save_seg_color write every frame's remapped map to out_dir/segmentation/<index>_label.png / _color.png (coloured with
--palette; a shard writes its own frames) and the style's to style_seg_label.png / style_seg_color.png.  --seg_size S
segments a bicubic downscale (long edge S) of the style and of every frame - made on the card, on the frame's stream - and samples
the logits at the stylised size ("Working resolution").  It excludes
--content_seg_dir, --content_seg / --style_seg, several --styles, --alpha_s_end and --interpolate_labels.
--seg_window W (2..8; an extension, the reference segments every frame on its own) takes a frame's labels from the mean of the
logits of the frame and of the W - 1 frames before it, weighted by --seg_decay D to the power of the age (1.0: uniform), so
that pixels between two close classes stop changing label from frame to frame ("Temporal window").  The first frames
of a clip use the frames that exist.  A shard that starts inside the clip also decodes the W - 1 frames before its first one and
segments them (only), so --shard / --gpus N write the frames and maps of one process.  The saved label maps are the windowed
ones, and the closing line reports the mean share of pixels whose saved label differs from the previous frame's.
--strength_map FILE (image_transfer.py's flag): one grey-scale map for every frame of the clip, white =
full stylisation, black = the untouched frame.  It is resized to the stylised frame size once per size and bound once
(cWCT.bind_strength); the blend y = x + s (A(x) - x) runs inside the kernels that apply a frame's cWCT while the decoder pass
loads its state.  It works on every route above, and the children of --gpus N get the flag unchanged.
--strength_dir DIR gives every frame a map of its own (a matte that follows a moving subject): one grey image per frame, sorted
by name, as many as frames, read as 8-bit grey by the decode workers next to their frames.  With --resize host a worker resizes
its matte (PIL BILINEAR) to the stylised size; with --resize device the matte goes up at its own size and is resized on the
frame's stream (the same bytes; a shrink past 16x per axis stays on the host, one line on stderr).  The frame's map is made on
the card, in the frame's stream (cWCT.frame_strength: one launch, nothing synchronises).  It excludes --strength_map.
--strength_labels SPEC [--strength_default D] gives labels of the frame's OWN label map a strength each ("12:0.2,20:0"; every
other label D, default 1): the map of --content_seg / --content_seg_dir, or --auto_seg's (windowed under --seg_window) before any
remapping.  It multiplies --strength_map / --strength_dir.  A shard reads only its own mattes; children of --gpus N get the
flags unchanged.
--style_map FILE (with two --styles) / --style_maps F_0 ... (one per style) are image_transfer.py's flags (DESIGN.md section 5,
"Style maps"): which style goes where, one set of planes for every frame of the clip.  The planes are resized to the stylised
frame size once per size and bound once (cWCT.bind_style_map); the styles are encoded and prefactored once, a frame costs K
factor launches and the mix apply inside its decoder pass.  They replace --alpha_s / --alpha_s_end, exclude every mask flag and
--auto_seg, and work with --alpha_c, --strength_map, --strength_dir, --preserve_luminance, --resize device, --shard and
--gpus N (children get the flags unchanged).
--style_map_dir DIR (with two --styles) / --style_maps_dirs D_0 ... D_{K-1} (one directory per style) give every frame a style
map of its own, for regions that move (a dancer in one style in front of a stage in another, a wipe that travels): one grey
image per frame and directory, sorted by name, as many as frames, the j-th file of every directory belonging to frame j; read
as 8-bit grey by the decode workers next to their frames.  --style_map_dir holds the weight of the second style; K directories
are mixed by v_k / sum_j v_j.  With --resize host a worker resizes the planes (PIL BILINEAR) to the stylised size; with
--resize device they go up at their own size and are resized on the frame's stream (the same bytes; a shrink past 16x per axis
stays on the host, one line on stderr).  The frame's map is made on the card, in the frame's stream (cWCT.frame_style_map: one
launch, nothing synchronises).  The planes of one frame must have one size.  A frame with a pixel at which every plane is 0
ends the run with a message that names the frame and its files, once the frame retires.  They exclude --style_map /
--style_maps and whatever those exclude, and --synthetic_motion; a shard reads only its own frames' planes, children of
--gpus N get the flags unchanged.
--stats_window W (2..8; an extension, the reference whitens every frame with its own statistics, :160-214) whitens a frame with
the statistics of the frame and of the W - 1 frames before it, weighted by --stats_decay D to the power of the age: the affine
map of cWCT is global to the frame, so without it a bright object that enters recolours the static background too (DESIGN.md
section 5, "Statistics window").  --stats_cut T ends a frame's window at the first older frame whose statistics lie further
than T x tr(C) away: a scene cut, so that nothing from before it reaches the frames after it.  It works on the unmasked and the
static-mask (--content_seg / --style_seg) routes with every option above that those routes take; not with --content_seg_dir or
--auto_seg.  A shard that starts inside the clip also decodes and encodes (only) the W - 1 frames before its first one, so
--shard / --gpus N write the frames of one process.  --map_drift reports the mean relative change of the affine map from one
frame to the next in the closing line, with any window.
--stats_by_label takes --stats_window to the per-frame label maps of --content_seg_dir and --auto_seg (with or without
--seg_window): every label's statistics are pooled over the frames of the window that hold the label, whatever slot it sat in
("Statistics window by label").  A frame with more than 8 valid labels is done again from its own
statistics, as without the window.  A shard also works through the (Ws - 1) + (Wt - 1) frames before its first one, with
their maps, so --shard / --gpus N write the frames of one process.  Not with --map_drift.  The closing line reports the mean
number of frames a live label pooled.
--video clip.y4m reads a YUV4MPEG2 file (vstnet_amd/y4m.py: 8-bit progressive C420jpeg / C420mpeg2 / C420 / C444; needs no
cv2), and a .y4m input - or --out_format y4m with a frame directory - writes out_dir/<clip>_<style>.y4m at the writer size: raw
video in, raw video out, no codec ("Raw video edge").  A frame's planes go up as the 1.5 bytes per pixel
they are on disk and are converted to RGB on the frame's stream (vstnet_amd/yuv.py), the stylised frame is converted back on
the card and written by one ordered sink thread.  A y4m input is always resized on the card (--resize device; one stderr line
if --resize host was in force, and an error - no host fallback - for a frame outside the device resize's limits).
--yuv_matrix {auto,bt601,bt709} (auto: bt709 from 1280 wide or above 576 high, else bt601) and --yuv_range {auto,limited,full}
(auto: the header's XCOLORRANGE, else limited) describe a y4m input, whose output takes the same spec and layout; with a frame
directory they describe the output (C420jpeg).  The rate is --fps, or the input's when --fps is not given.  --shard i/n writes a
headerless part out_dir/<clip>_<style>/part_<rank>.yuv and the parent of --gpus N joins the parts behind one header
(y4m.merge_parts): the bytes one process writes.  Every other option keeps working and keeps reading images from its directory.
--video clip.yuv --pix_fmt F --video_size WxH [--fps N] [--yuv_siting left|centre] reads a headerless raw YUV file
(vstnet_amd/rawyuv.py): yuv420p, yuv444p, or yuv420p / yuv422p / yuv444p with 9, 10, 12, 14 or 16 bits, little-endian - what
`ffmpeg -f rawvideo -pix_fmt yuv420p10le` writes and HM, VTM, x265 and SVT-AV1 read.  A high-bit-depth frame goes up as the
bytes it is on disk, is converted to float planes on the frame's stream and enters the encoder as those; the decoder's float
planes are converted back at the target depth (vstnet_amd/yuv.py; DESIGN.md section 6, "High-bit-depth edge"): nothing passes
through 256 levels.  The output is out_dir/<clip>_<style>_<W>x<H>_<pix_fmt>.yuv in the input's pix_fmt.  --out_format yuv writes
a raw file behind any input (yuv420p unless --out_pix_fmt says otherwise), and --out_pix_fmt F writes a raw file of that format
behind ANY input - a frame directory or an 8-bit .y4m included, e.g. 8-bit frames in, yuv420p10le out - while the input side
stays what it is.  Deep output is always a raw file, never a y4m.  --yuv_matrix / --yuv_range apply as for y4m (range auto:
limited; the output takes the input's).  A high-bit-depth input of any size is resized on the card with --resize device: the
planes go up at the source size and img_resize restated in float, fused with the conversion, makes the encoder's float planes and
their 8-bit twin at the stylised size (vstnet_amd/yuv.py DeepImgResize; DESIGN.md section 6, "Deep resize"; a step may shrink an
axis by 16 at the most, no host fallback).  With --resize host it must pass the resize rule unchanged - long edge at most
--max_size, both edges multiples of 4 -: the host float resize is not built yet.  An 8-bit raw input is resized
on the card like a y4m.  --shard i/n writes out_dir/<clip>_<style>/part_<rank>.yuv and the parent of --gpus N joins the parts
(rawyuv.merge_parts).  Every other option keeps working: --auto_seg, label strengths and mattes read the frame's 8-bit twin,
which the conversion writes next to the float planes, and --preserve_luminance blends on the float planes.
--upscale guided (an extension; DESIGN.md section 6, "Guided upscale"; default bicubic: nothing changes) writes every frame at
the SOURCE frame's size instead of the writer size: the frame is stylised at the working size as always, a colour guided filter
fits the stylised frame as a locally affine function of the resized content, and the fitted coefficients are sampled at the full
size and applied to the source frame on the card (vstnet_amd/guided.py), so edges and texture come from the source.
--upscale_radius R (1..8, default 4) and --upscale_eps E (> 0, default 1e-3) are the filter's window and ridge: starting values,
picture quality has not been measured.  It needs --resize device, 8-bit input and output and --mode photorealistic (the
artistic model is not trained to be locally affine); a clip whose frames are not resized at all has nothing to upscale and takes
the plain path (one stderr line).  Everything that acts before the decoder keeps working, and the step has no state across
frames, so --shard / --gpus N write the bytes of one process.

--affinity (an extension; DESIGN.md section 6, "Affinity loss"; off: nothing changes) measures every frame's Matting-Laplacian
loss - the reference's training measure of photorealism, how far the stylised frame is from a locally affine function of its
content in every window - on the card (vstnet_amd/matting.py) and writes out_dir/<clip>_<style>/affinity.csv, one line per frame:
index,loss_work[,loss_full].  loss_work is taken at the working size: on the decoded uint8 frame against the resized content,
or, under --upscale guided, on the decoder's float frame; loss_full, under --upscale guided only, on the written full-size frame
against the source frame.  The closing line gives mean, max and the frame of the max.  --affinity_radius R (1..3, default 1) and
--affinity_eps E (default 1e-7) are the reference's win_rad and eps.  --shard i/n writes affinity.part<i>.csv and the parent of
--gpus N joins the parts into the file one process writes.  Not with a high-bit-depth output, and a clip whose frames are
written at another size than they are stylised at needs --upscale guided.  The written frames are those without the flag.

--style_loss (an extension; DESIGN.md section 6, "Style loss"; off: nothing changes) measures how much of the style survived:
the reference's VGG-19 style loss (loss_s of models/VGG.py: the means and standard deviations of relu1_1 .. relu4_1) of every
WRITTEN frame against the style image, on the card (vstnet_amd/vgg.py), written to out_dir/<clip>_<style>/style.csv, one line
per frame: index,loss_s[,loss_c].  --content_loss adds the reference's content loss (relu4_1 of the written frame against that
of its content frame; the written size must be the stylised size).  Every instrument above is at its best when the content
frame is written back unchanged; this one is the counterweight.  The weights come from --vgg_ckpoint PATH (the reference's
vgg_normalised.pth) or --synthetic_vgg_weights (seeded stand-ins: the values then show that the instrument works and nothing
more).  Under --styles the style records are those of the first style.  The closing line gives mean, max and the frame of the
max; --shard i/n writes style.part<i>.csv and the parent of --gpus N joins the parts.  Not with a high-bit-depth output.  The
written frames are those without the flag.

--temporal (an extension; DESIGN.md section 6, "Temporal loss"; off: nothing changes) measures flicker under known motion, the
reference's temporal loss (utils/TemporalLoss.py): for every frame with a predecessor, mean |warp(frame t-1, flow t) - frame t|
of the stylised pair (loss_out) and of the input pair (loss_in), on the card (vstnet_amd/temporal.py), written to
out_dir/<clip>_<style>/temporal.csv, one line per frame: index,loss_out,loss_in (empty cells where there is no value).  The
closing line gives both means, their ratio (how much the stylisation amplifies the input's own frame difference), the max and
its frame.  The motion comes from one of three sources.  --flow_dir DIR: one .flo (Middlebury) or .npy ([2,H,W] float32) file per
frame transition, sorted by name, n_frames - 1 of them, at the stylised size; file j holds f such that frame j sampled at
x - f(x) predicts frame j+1 (the reference's convention; --flow_negate for files that hold the opposite sign).
--synthetic_motion N: --video names ONE image; it is resized by the host rule (utils.utils.img_resize) whatever --resize says -
the clip is made at the stylised size, so no frame of it is resized again - and N frames with known motion are made from it on
the card (vstnet_amd.temporal.synthetic_clip: the reference's GenerateFakeData chained; --motion_level 8 --shift_level 10
--noise_level 0.001 --motion_seed 0) and stylised as a clip.
--estimate_flow: the flow of every frame pair is estimated on the card from the INPUT frames (vstnet_amd/flow.py: a coarse-to-fine,
warping Lucas-Kanade scheme in fp64; --flow_levels 5 --flow_iters 3 --flow_radius 3 --flow_lambda 1e-3 are starting values checked
on synthetic textures only); it works on every route --flow_dir works on.  --flow_mask also estimates the backward flow, counts only
the pixels where the two agree (the forward-backward check: disoccluded pixels are not flicker) and adds a fourth column, the
share of such pixels.
--temporal does not go with --shard / --gpus N (a shard's first frame needs its
neighbour's output), --upscale guided, a high-bit-depth output, or a clip written at another size than it is stylised at;
--synthetic_motion also excludes --content_seg, --content_seg_dir and --strength_dir, whose maps would have to move with the
frames.  All of these are argparse errors (exit status 2) before anything is read, except two that need the first frame: the
written size against the stylised one, and the number of flow files against the number of frames; they come once the clip has
been opened, before anything is stylised.  The written frames are those without the flag.
--stabilise [GAIN] (with --temporal, any of its motion sources; DESIGN.md section 6, "Stabiliser") is the one flag here that
changes the written frames: every frame with a predecessor and a flow is blended, behind its decode, with the frame WRITTEN before
it sampled along the flow, with a weight GAIN / (1 + e / sigma^2) that falls off where the input pair changed along that flow
(--stabilise_sigma 8, in levels) and a step of at most --stabilise_limit 24 levels per byte; with --flow_mask the masked-out
pixels are left alone.  temporal.csv's loss_out is then that of the written frames, and stabilise.csv next to it holds
index,loss_raw,loss_out - the decoder's pairs against the written ones - with a closing line of both means and their ratio.
GAIN 0.7, sigma 8 and limit 24 are starting values from a numpy prototype on constructed clips: picture quality on real footage
is unmeasured.  It excludes --content_seg_dir and --auto_seg (a frame done again would leave a stale frame in the recursion),
and whatever --temporal excludes.
"""
import sys
import argparse
import os
import re

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from image_transfer import (build_network, add_mix_arguments, check_mix_args, add_seg_arguments, check_seg_args,
                            build_segmenter, device_remapper, save_seg_maps, check_seg_pixels, segment_image,
                            add_strength_argument, check_strength_args, load_strength_map, load_matte,
                            add_style_map_arguments, check_style_map_args, check_style_map_planes, load_style_map, MAX_STYLES)
from utils.utils import img_resize, load_segment, to_tensor_u8
from vstnet_amd.pipeline import FramePipeline, AsyncSink, StyleMapZeroSum, prefetch, parallel_map, host_workers, save_png
from vstnet_amd.sharding import shard_range

IMG_EXT = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp')


def build_parser():
    p = argparse.ArgumentParser(allow_abbrev=False)     # (an abbreviated --gpu would survive launch_shards' argv rewrite)
    p.add_argument('--mode', type=str, default='photorealistic')
    p.add_argument('--ckpoint', type=str, default='checkpoints/photo_video.pt')
    p.add_argument('--video', type=str, default='data/content/03.avi')
    p.add_argument('--style', type=str, default='data/style/03.jpeg')
    p.add_argument('--out_dir', type=str, default="output")
    p.add_argument('--max_size', type=int, default=1280)
    p.add_argument('--alpha_c', type=float, default=None)
    p.add_argument('--fps', type=int, default=None, help="default 30, or the rate of a .y4m input")
    p.add_argument('--content_seg', type=str, default=None, help="one label map used for every frame")
    p.add_argument('--content_seg_dir', type=str, default=None, help="one label map per frame (sorted by name, as many as "
                   "frames): RGB maps in the dictionary colours, or single-channel (L / P) PNGs taken as labels")
    p.add_argument('--seg_remap', action='store_true', default=False, help="with --content_seg_dir: self_remapping of the style "
                   "map, self_remapping + cross_remapping of every frame's map (the reference's --auto_seg post-processing)")
    p.add_argument('--label_mapping', type=str, default='models/segmentation/ade20k_semantic_rel.npy')
    p.add_argument('--min_ratio', type=float, default=0.01)
    p.add_argument('--style_seg', type=str, default=None)
    p.add_argument('--auto_seg', action='store_true', default=False)
    p.add_argument('--synthetic_weights', action='store_true', default=False)
    p.add_argument('--shard', type=str, default="0/1")
    p.add_argument('--gpus', type=int, default=1, help="start this many child processes, one GPU each, and merge their outputs")
    p.add_argument('--precision', type=str, default=None, help="conv arithmetic (default: the library's, bf16x3)")
    p.add_argument('--frames_only', action='store_true', default=False, help="write numbered PNGs even if cv2 is there "
                   "(what the children of --gpus N do: the parent encodes the one clip)")
    p.add_argument('--stub_stylise', action='store_true', default=False, help=argparse.SUPPRESS)   # host-logic tests: no GPU
    p.add_argument('--depth', type=int, default=4, help="pinned ring slots (frames queued ahead of the one being written)")
    p.add_argument('--streams', type=int, default=3, help="frames in flight on the card (1080p, 5-label masks, files in -> PNGs out: "
                   "89 / 102 / 103 frames/s at 2 / 3 / 4, profiles/r04_other_configs.jsonl)")
    p.add_argument('--workers', type=int, default=0, help="host threads that decode + resize input frames, and as many that "
                   "encode output frames (0: a share of this process's cores); the GPU loop itself is one thread")
    p.add_argument('--resize', type=str, default='host', choices=('host', 'device'), help="where a frame is resized: host = PIL on "
                   "the decode threads (and torch ops for the resize to the writer size); device = the decode threads hand over "
                   "the decoded frame and both resizes run as HIP kernels on the frame's stream (vstnet_amd/resize.py: the input "
                   "side gives PIL's bytes, the output side is within one count of the host path).  A high-bit-depth raw input "
                   "that does not pass the resize rule unchanged needs device: its planes are resized in float on the card "
                   "(there is no host float resize)")
    p.add_argument('--upscale', type=str, default='bicubic', choices=('bicubic', 'guided'), help="bicubic: the stylised frame is "
                   "resized to the writer size (the default, unchanged); guided: the frame is written at the source frame's size "
                   "- a colour guided filter fitted at the working size carries the stylisation over to the source frame on the "
                   "card (vstnet_amd/guided.py).  Needs --resize device, 8-bit input and output, --mode photorealistic")
    p.add_argument('--upscale_radius', type=int, default=4, help="--upscale guided: the window radius at the working size, 1..8 "
                   "(a starting value: picture quality has not been measured)")
    p.add_argument('--upscale_eps', type=float, default=1e-3, help="--upscale guided: the ridge added to the guide's covariance, "
                   "> 0 (a starting value, as above)")
    p.add_argument('--preserve_luminance', action='store_true', default=False, help="keep each frame's Lab luminance, take the "
                   "stylised chroma (as image_transfer.py --preserve_luminance), on the device, with every other option; "
                   "--stub_stylise (the host-logic rehearsal, which stylises nothing) accepts the flag and ignores it")
    add_seg_arguments(p)
    p.add_argument('--seg_window', type=int, default=1, metavar='W', help="--auto_seg: label every frame from the mean logits of "
                   "the frame and of the W - 1 frames before it (1..8; 1 = every frame on its own)")
    p.add_argument('--seg_decay', type=float, default=1.0, metavar='D', help="--seg_window: a frame of age k weighs D**k "
                   "(0 < D <= 1; 1.0 = a uniform window)")
    p.add_argument('--stats_window', type=int, default=1, metavar='W', help="whiten every frame with the content statistics of "
                   "the frame and of the W - 1 frames before it (1..8; 1 = every frame on its own, the reference's behaviour)")
    p.add_argument('--stats_by_label', action='store_true', default=False, help="--stats_window under per-frame label maps "
                   "(--content_seg_dir or --auto_seg): pool every label's statistics over the frames that hold the label")
    p.add_argument('--stats_decay', type=float, default=None, metavar='D', help="--stats_window: the statistics of a frame of age k "
                   "weigh D**k (0 < D <= 1; default 1.0 = the statistics of the union of the frames' pixels)")
    p.add_argument('--stats_cut', type=float, default=None, metavar='T', help="--stats_window: a scene cut ends the window - the "
                   "first older frame with |mean - mean_0|^2 + |C - C_0|_F > T x tr(C_0), and every frame before it, is left out "
                   "(>= 0; default 0 = off).  No recommended value has been measured on real footage; on synthetic codes "
                   "near-duplicate frames sit near 1e-3 and different scenes at 0.1-0.4")
    p.add_argument('--affinity', action='store_true', default=False, help="measure every frame's Matting-Laplacian loss against its "
                   "content frame on the card (an extension; DESIGN.md section 6, \"Affinity loss\"): affinity.csv next to the "
                   "frames and a closing line; the written frames do not change")
    from vstnet_amd import style_files
    style_files.add_arguments(p)
    p.add_argument('--affinity_radius', type=int, default=1, help="--affinity: the window radius, 1..3 (the reference's win_rad)")
    p.add_argument('--affinity_eps', type=float, default=1e-7, help="--affinity: the ridge (the reference's eps), > 0")
    p.add_argument('--temporal', action='store_true', default=False, help="measure every frame pair's temporal loss (warping error "
                   "under known motion) on the card (an extension; DESIGN.md section 6, \"Temporal loss\"): temporal.csv next to the "
                   "frames and a closing line; needs --flow_dir or --synthetic_motion; the written frames do not change")
    p.add_argument('--flow_dir', type=str, default=None, metavar='DIR', help="--temporal: one .flo or .npy flow per frame "
                   "transition (sorted by name, n_frames - 1 of them, at the stylised size); file j maps frame j onto frame j+1.  "
                   "Their number, like the written size against the stylised one, is checked once the clip has been opened")
    p.add_argument('--flow_negate', action='store_true', default=False, help="--flow_dir: the files hold the opposite sign")
    p.add_argument('--estimate_flow', action='store_true', default=False, help="--temporal: estimate every frame pair's flow on the "
                   "card from the input frames (coarse-to-fine Lucas-Kanade; an extension; DESIGN.md section 6, \"Optical flow\"): "
                   "the motion source for footage that comes without flow files")
    p.add_argument('--flow_levels', type=int, default=5, help="--estimate_flow: pyramid levels, 1..8")
    p.add_argument('--flow_iters', type=int, default=3, help="--estimate_flow: iterations per level, 1..16")
    p.add_argument('--flow_radius', type=int, default=3, help="--estimate_flow: window radius, 1..7")
    p.add_argument('--flow_lambda', type=float, default=1e-3, help="--estimate_flow: the regulariser of the 2x2 system, > 0")
    p.add_argument('--flow_mask', action='store_true', default=False, help="--estimate_flow: also estimate the backward flow and count "
                   "only the pixels where the two agree (forward-backward check); temporal.csv gets a fourth column, the share "
                   "of such pixels")
    p.add_argument('--stabilise', type=float, nargs='?', const=0.7, default=None, metavar='GAIN', help="--temporal: blend every "
                   "frame, before it is written, with the frame written before it sampled along the flow, where the input did "
                   "not change along that flow (an extension; DESIGN.md section 6, \"Stabiliser\"); GAIN in (0, 1), 0.7 when "
                   "given bare; stabilise.csv next to temporal.csv.  The three values are starting values: picture quality is "
                   "unmeasured")
    p.add_argument('--stabilise_sigma', type=float, default=8.0, help="--stabilise: the input change along the flow, in levels "
                   "(root mean square over the channels), at which the blend weight halves; > 0")
    p.add_argument('--stabilise_limit', type=float, default=24.0, help="--stabilise: the most a byte may move, in levels; >= 0")
    p.add_argument('--synthetic_motion', type=int, default=None, metavar='N', help="--temporal: --video names one image; it is resized "
                   "by the host rule whatever --resize says, and N frames with known motion are made from it on the card at the "
                   "stylised size (N >= 2)")
    p.add_argument('--motion_level', type=float, default=8, help="--synthetic_motion: the deviation of the coarse flow grid, pixels")
    p.add_argument('--shift_level', type=int, default=10, help="--synthetic_motion: the largest whole-frame shift per axis, pixels")
    p.add_argument('--noise_level', type=float, default=0.001, help="--synthetic_motion: the noise added to every frame (of 0..1)")
    p.add_argument('--motion_seed', type=int, default=0, help="--synthetic_motion: the seed of every draw")
    p.add_argument('--map_drift', action='store_true', default=False, help="report the mean relative change of the frames' affine "
                   "maps, |a_t - a_(t-1)| / |a_t|, in the closing line (any --stats_window)")
    p.add_argument('--out_format', type=str, default='auto', choices=('auto', 'y4m', 'yuv'), help="y4m: write "
                   "out_dir/<clip>_<style>.y4m (YUV4MPEG2, uncompressed); yuv: write a headerless raw file "
                   "out_dir/<clip>_<style>_<W>x<H>_<pix_fmt>.yuv; auto: y4m for a .y4m input, yuv for a .yuv input, else an .mp4 "
                   "with cv2 / numbered PNGs without")
    p.add_argument('--pix_fmt', type=str, default=None, metavar='F', help="the sample format of a raw .yuv input: yuv420p, yuv444p, "
                   "or yuv420p / yuv422p / yuv444p with 9, 10, 12, 14 or 16 bits, little-endian (yuv420p10le)")
    p.add_argument('--video_size', type=str, default=None, metavar='WxH', help="the frame size of a raw .yuv input")
    p.add_argument('--yuv_siting', type=str, default='left', choices=('left', 'centre'), help="where the chroma samples of raw "
                   "4:2:0 planes sit horizontally: left = on the even luma columns (MPEG-2, H.264, HEVC), centre = between them")
    p.add_argument('--out_pix_fmt', type=str, default=None, metavar='F', help="write a raw .yuv file of this sample format, "
                   "whatever the input is (8-bit frames in, yuv420p10le out)")
    p.add_argument('--yuv_matrix', type=str, default='auto', choices=('auto', 'bt601', 'bt709'), help="the Y'CbCr matrix of a "
                   ".y4m input and of the y4m output (auto: bt709 from 1280 wide or above 576 high, else bt601)")
    p.add_argument('--yuv_range', type=str, default='auto', choices=('auto', 'limited', 'full'), help="the code range of a .y4m "
                   "input and of the y4m output (auto: the input header's XCOLORRANGE, else limited)")
    add_mix_arguments(p)
    add_strength_argument(p)
    add_style_map_arguments(p)
    p.add_argument('--style_map_dir', type=str, default=None, metavar='DIR', help="with two --styles: one grey-scale map per frame "
                   "(sorted by name, as many as frames), per pixel the weight of the SECOND style, as --style_map for one frame")
    p.add_argument('--style_maps_dirs', type=str, nargs='+', default=None, metavar='DIR', help="with K --styles: one directory per "
                   "style, each with one grey-scale map per frame (sorted by name); frame j mixes the styles by the j-th files, "
                   "v_k / sum_j v_j, as --style_maps for one frame")
    p.add_argument('--strength_dir', type=str, default=None, metavar='DIR', help="one grey-scale map per frame (sorted by name, as "
                   "many as frames), read as 8-bit grey: white = full stylisation, black = the untouched frame")
    p.add_argument('--alpha_s_end', type=float, nargs='+', default=None, help="the weights of the clip's last frame: the mix "
                   "moves linearly from --alpha_s (first frame) to these")
    p.add_argument('--png_level', type=int, default=0, help="numbered PNGs (the output without cv2, and the shard -> parent "
                   "hand-off of --gpus N): 0 = stored rows, a few ms per 1080p frame, 3 bytes per pixel; 1-9 = PIL's filters + "
                   "zlib at that level (about 30 %% smaller on photographs, 10-30x the encode time).  Lossless either way")
    return p


class FrameDir:
    """A directory of frames as a lazy sequence: a frame is decoded when it is asked for, so a shard (one of N processes) holds
    only its own frames and the parent of a multi-GPU run only the first one (for the writer size)."""

    def __init__(self, path):
        self.files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(IMG_EXT))

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        return Image.open(self.files[i]).convert('RGB')


def check_raw_args(parser, args):
    """--pix_fmt / --video_size / --out_pix_fmt, checked before anything is read: argparse errors (exit status 2, usage on stderr).
    Returns the (width, height) of a raw .yuv input, or None for any other input."""
    from vstnet_amd.rawyuv import parse_pix_fmt
    for flag in ("pix_fmt", "out_pix_fmt"):
        if getattr(args, flag) is not None:
            try:
                parse_pix_fmt(getattr(args, flag))
            except ValueError as e:
                parser.error("--%s: %s" % (flag, e))
    if args.out_pix_fmt is not None and args.out_format == 'y4m':
        parser.error("--out_pix_fmt writes a raw .yuv file: not with --out_format y4m")
    if os.path.isdir(args.video) or not args.video.lower().endswith(".yuv"):
        if args.pix_fmt is not None or args.video_size is not None:
            parser.error("--pix_fmt and --video_size describe a raw .yuv input (--out_pix_fmt names the output's format)")
        return None
    if args.pix_fmt is None or args.video_size is None:
        parser.error("a raw .yuv input carries no header: it needs --pix_fmt and --video_size WxH")
    m = re.match(r"^(\d+)[xX](\d+)$", args.video_size)
    if m is None or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        parser.error("--video_size is WxH, e.g. 1920x1080; got %r" % args.video_size)
    return int(m.group(1)), int(m.group(2))


def read_frames(path):
    if os.path.isdir(path):
        return FrameDir(path)
    if path.lower().endswith(".y4m"):
        from vstnet_amd.y4m import Y4MClip
        return Y4MClip(path)
    try:
        import cv2
    except ImportError as e:
        raise RuntimeError("reading a video file needs cv2; pass a directory of frames or a .y4m file instead") from e
    frames, cap = [], cv2.VideoCapture(path)
    while True:
        ret, frame = cap.read()
        if ret is False:
            break
        frames.append(Image.fromarray(frame[..., ::-1]))
    return frames


def writer_size(first_frame, max_size):
    """video_transfer.py:82-86, including its overwrite-before-use quirk.  first_frame: an image, or its (width, height)."""
    if isinstance(first_frame, tuple):
        video_width, video_height = first_frame
    else:
        video_height, video_width = np.array(first_frame).shape[:2]
    if max(video_width, video_height) > max_size:
        video_width = int(1.0 * video_width / max(video_width, video_height) * max_size)
        video_height = int(1.0 * video_height / max(video_width, video_height) * max_size)
    return video_width, video_height


def clip_name(args):
    return "%s_%s" % (os.path.basename(args.video.rstrip("/")).split(".")[0], os.path.basename(args.style).split(".")[0])


FRAME_PNG = re.compile(r"^\d{5}\.png$")

LAST_RUN = {}        # what the last main() of this process did: {"masks": {frame index: map file}, "redo": frames done again}


def check_window_args(parser, args):
    """--seg_window / --seg_decay, checked before any GPU work: argparse errors (exit status 2, usage on stderr)."""
    from vstnet_amd.segformer import MAX_WINDOW
    if not 1 <= args.seg_window <= MAX_WINDOW:
        parser.error("--seg_window must be in 1..%d" % MAX_WINDOW)
    if not 0.0 < args.seg_decay <= 1.0:
        parser.error("--seg_decay must be in (0, 1]")
    if args.seg_window > 1 and not args.auto_seg:
        parser.error("--seg_window filters the logits of --auto_seg (the maps of --content_seg_dir come from files)")


def check_stats_args(parser, args):
    """--stats_window / --stats_decay / --stats_cut, checked before any GPU work: argparse errors (exit status 2, usage on
    stderr).  Fills the defaults of the two companions in."""
    from vstnet_amd._lib import STATS_POOL_MAX
    if not 1 <= args.stats_window <= STATS_POOL_MAX:
        parser.error("--stats_window must be in 1..%d" % STATS_POOL_MAX)
    if args.stats_window == 1 and (args.stats_decay is not None or args.stats_cut is not None):
        parser.error("--stats_decay and --stats_cut belong to --stats_window W with W > 1")
    if args.stats_decay is not None and not 0.0 < args.stats_decay <= 1.0:
        parser.error("--stats_decay must be in (0, 1]")
    if args.stats_cut is not None and not 0.0 <= args.stats_cut < float("inf"):
        parser.error("--stats_cut must be >= 0")
    per_frame_maps = args.content_seg_dir is not None or args.auto_seg
    if args.stats_by_label:
        if args.stats_window == 1:
            parser.error("--stats_by_label belongs to --stats_window W with W > 1")
        if not per_frame_maps:
            parser.error("--stats_by_label pools by label under per-frame label maps: it needs --content_seg_dir or --auto_seg "
                         "(one map for the clip, --content_seg, has the same slots in every frame: --stats_window alone)")
        if args.map_drift:
            parser.error("--map_drift does not go with --stats_by_label: the slot order changes from frame to frame")
    elif args.stats_window > 1 and per_frame_maps:
        parser.error("--stats_window pools the statistics of a fixed set of label slots: not with --content_seg_dir or --auto_seg "
                     "(their slots differ from frame to frame) unless --stats_by_label lines the records up by label")
    args.stats_decay = 1.0 if args.stats_decay is None else args.stats_decay
    args.stats_cut = 0.0 if args.stats_cut is None else args.stats_cut


def warmup_range(start, window):
    """The frames a run that starts at frame `start` segments without stylising them: the up to window - 1 frames before it."""
    return tuple(range(max(0, start - window + 1), start))


def warmup_frames(start, seg_window, stats_window):
    """The frames a run that starts at frame `start` works through without writing them.  --seg_window Ws and --stats_window Wt
    together (--stats_by_label): the Wt - 1 frames before `start` for their statistics and the Ws - 1 before those for the
    logits behind their labels (vstnet_amd.pipeline.warmup_counts has the split).  One window alone: its W - 1 frames."""
    return warmup_range(start, (seg_window - 1) + (stats_window - 1) + 1)


class FlickerMeter:
    """The mean share of pixels whose label differs from the previous frame's, over the maps one process writes (called in
    frame order; a frame of another size starts over)."""

    def __init__(self):
        self.prev, self.total, self.pairs = None, 0.0, 0

    def __call__(self, m):
        if self.prev is not None and self.prev.shape == m.shape:
            self.total += float(np.count_nonzero(self.prev != m)) / m.size
            self.pairs += 1
        self.prev = np.array(m, copy=True)

    @property
    def share(self):
        return self.total / self.pairs if self.pairs else 0.0


def check_mask_args(args, n_frames):
    """--content_seg_dir and its companions, checked before any GPU work (and before any child is started): the sorted map
    files, or None without per-frame maps."""
    if args.content_seg_dir is None:
        if args.seg_remap:
            raise SystemExit("--seg_remap post-processes the per-frame maps of --content_seg_dir")
        return None
    if args.content_seg is not None:
        raise SystemExit("--content_seg_dir (one map per frame) and --content_seg (one map for every frame) are mutually exclusive")
    if args.mode != 'photorealistic':
        raise SystemExit("--content_seg_dir needs --mode photorealistic (masked artistic codes have no per-frame route)")
    if args.style_seg is None:
        raise SystemExit("--content_seg_dir needs --style_seg")
    if not os.path.isdir(args.content_seg_dir):
        raise SystemExit("--content_seg_dir %s is not a directory" % args.content_seg_dir)
    files = sorted(os.path.join(args.content_seg_dir, f) for f in os.listdir(args.content_seg_dir) if f.lower().endswith(IMG_EXT))
    if len(files) != n_frames:
        raise SystemExit("--content_seg_dir holds %d maps for %d frames: one map per frame is needed" % (len(files), n_frames))
    if args.seg_remap and not os.path.exists(args.label_mapping):
        raise SystemExit("--seg_remap needs the relation table (--label_mapping %s not found)" % args.label_mapping)
    return files


def check_strength_dir(parser, args, n_frames):
    """--strength_dir, checked before any GPU work (and before any child is started): the sorted matte files, or None."""
    if args.strength_dir is None:
        return None
    if args.strength_map is not None:
        parser.error("--strength_dir (one map per frame) and --strength_map (one map for every frame) are mutually exclusive")
    if not os.path.isdir(args.strength_dir):
        parser.error("--strength_dir %s is not a directory" % args.strength_dir)
    files = sorted(os.path.join(args.strength_dir, f) for f in os.listdir(args.strength_dir) if f.lower().endswith(IMG_EXT))
    if len(files) != n_frames:
        parser.error("--strength_dir holds %d maps for %d frames: one map per frame is needed" % (len(files), n_frames))
    return files


class StylePlanesError(ValueError):
    """The planes --style_map_dir / --style_maps_dirs give one frame cannot be used: main ends the run with the message."""


def check_style_map_dir_args(parser, args):
    """--style_map_dir / --style_maps_dirs, what the command line alone decides, before check_mix_args fills the defaults in:
    argparse errors (exit status 2) before any GPU work and before any child is started.  The list of directories, or None."""
    if args.style_map_dir is None and args.style_maps_dirs is None:
        return None
    if args.style_map_dir is not None and args.style_maps_dirs is not None:
        parser.error("--style_map_dir (one directory, two styles) and --style_maps_dirs (one directory per style) are mutually "
                     "exclusive")
    flag = "--style_map_dir" if args.style_map_dir is not None else "--style_maps_dirs"
    if args.style_map is not None or args.style_maps is not None:
        parser.error("%s (a map per frame) and --style_map / --style_maps (one map for every frame) are mutually exclusive" % flag)
    dirs = [args.style_map_dir] if args.style_map_dir is not None else list(args.style_maps_dirs)
    n = len(args.styles) if args.styles is not None else 1
    if args.style_map_dir is not None and n != 2:
        parser.error("--style_map_dir holds the weight of the second of two styles: it needs --styles A B (got %d style%s); "
                     "--style_maps_dirs takes one directory per style" % (n, "" if n == 1 else "s"))
    if args.style_maps_dirs is not None and (len(dirs) != n or not 2 <= n <= MAX_STYLES):
        parser.error("--style_maps_dirs takes one directory per style for 2..%d --styles: %d directories for %d style%s"
                     % (MAX_STYLES, len(dirs), n, "" if n == 1 else "s"))
    if args.alpha_s is not None or args.alpha_s_end is not None:
        parser.error("%s takes the place of the styles' weights: it excludes --alpha_s / --alpha_s_end" % flag)
    masks = [f for f in ("content_seg", "content_seg_dir", "style_seg", "style_segs") if getattr(args, f, None) is not None]
    masks += [f for f in ("auto_seg", "interpolate_labels", "seg_remap") if getattr(args, f, False)]
    if masks or args.strength_labels is not None:
        parser.error("%s: style maps are not supported on the masked routes (it excludes --%s)"
                     % (flag, (masks + ["strength_labels"])[0]))
    if args.synthetic_motion is not None:
        parser.error("--synthetic_motion moves the frames, and the maps of %s would have to move with them: not together" % flag)
    for d in dirs:
        if not os.path.isdir(d):
            parser.error("%s %s is not a directory" % (flag, d))
    return dirs


def check_style_map_dirs(parser, args, dirs, n_frames, size_wh):
    """The rest, once the clip is open and still before any GPU work: one map per frame in every directory, and frames that stay
    off the tiled route (size_wh: the first frame's stylised size).  Per directory the sorted files, or None without the flags."""
    if dirs is None:
        return None
    flag = "--style_map_dir" if args.style_map_dir is not None else "--style_maps_dirs"
    from vstnet_amd import tiled
    if tiled.needs_tiling(size_wh[1], size_wh[0], float("inf")):
        parser.error("%s does not work on the tiled route, which a %dx%d frame takes: lower --max_size" % (flag, size_wh[0], size_wh[1]))
    files = []
    for d in dirs:
        names = sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(IMG_EXT))
        if len(names) != n_frames:
            parser.error("%s %s holds %d maps for %d frames: one map per frame is needed" % (flag, d, len(names), n_frames))
        files.append(names)
    return files


def load_frame_mask(path, size_wh):
    """One frame's map, NEAREST-resized to the stylised frame size (load_segment's rule): uint8 [H,W] labels for a
    single-channel (L / P) file, else uint8 [H,W,3] colours - the dictionary lookup happens on the device."""
    img = Image.open(path)
    if img.mode not in ("L", "P"):
        img = img.convert("RGB")
    if img.size != tuple(size_wh):
        img = img.resize(tuple(size_wh), Image.NEAREST)
    return np.ascontiguousarray(np.asarray(img, dtype=np.uint8))


def mix_weights(args, i, n_frames):
    """The style weights of frame i (its GLOBAL index) of a clip of n_frames frames: --alpha_s, or the linear cross-fade from
    --alpha_s to --alpha_s_end."""
    if args.alpha_s_end is None:
        return list(args.alpha_s)
    t = i / (n_frames - 1) if n_frames > 1 else 0.0
    return [(1.0 - t) * a + t * b for a, b in zip(args.alpha_s, args.alpha_s_end)]


def launch_shards(args, argv):
    """--gpus N: N children, one per GPU, each on its contiguous shard; decided before this process touches a GPU (no torch.cuda
    call here: GPUs are counted from the visible-devices restriction / the KFD topology, vstnet_amd.sharding.count_gpus)."""
    from vstnet_amd.sharding import launch_children, rank_environment, count_gpus
    n = args.gpus
    base = [a for a in argv]
    for flag in ("--gpus", "--shard"):                  # children get their own --shard and `--gpus 1`
        while flag in base:
            i = base.index(flag)
            del base[i:i + 2]
    base = [a for a in base if not a.startswith("--gpus=") and not a.startswith("--shard=")]
    # (the explicit `--gpus 1` comes last and wins whatever survived the rewrite: a child never launches children)
    cmds = [[sys.executable, os.path.abspath(__file__)] + base + ["--shard", "%d/%d" % (r, n), "--frames_only", "--gpus", "1"]
            for r in range(n)]
    # numbered frames of an earlier (longer) run in the children's output directory would fail the merge only after every child
    # has done its work: they are this script's own outputs, so they go now; anything else in there is left alone
    frame_dir = os.path.join(args.out_dir, clip_name(args))
    if os.path.isdir(frame_dir):
        for f in os.listdir(frame_dir):
            if FRAME_PNG.match(f):
                os.remove(os.path.join(frame_dir, f))
    n_dev = count_gpus()
    return launch_children(cmds, [rank_environment(r, n, visible_device=True, n_devices=n_dev or None) for r in range(n)])


def merge_outputs(frame_dir, n_frames, out_dir, name, fps, size):
    """The host side of SURVEY 8(e): the shards wrote frame i as <frame_dir>/%05d.png; check that every index 0..n-1 is there
    exactly once, then — with cv2 — encode the ONE clip <out_dir>/<name>.mp4 in frame order (one lossy encode, like the
    reference's single writer) and drop the PNGs; without cv2 the ordered frame directory is the output."""
    have = sorted(f for f in os.listdir(frame_dir) if FRAME_PNG.match(f))      # (other files in there are not ours)
    want = ["%05d.png" % i for i in range(n_frames)]
    if have != want:
        missing = sorted(set(want) - set(have))
        extra = sorted(set(have) - set(want))
        raise RuntimeError(f"merge: {len(missing)} frames missing (first {missing[:3]}), {len(extra)} unexpected (first {extra[:3]})")
    try:
        import cv2
    except ImportError:
        return frame_dir
    path = os.path.join(out_dir, name + ".mp4")
    writer = cv2.VideoWriter(path, cv2.VideoWriter_fourcc('m', 'p', '4', 'v'), fps, size)
    try:
        for f in want:
            writer.write(np.asarray(Image.open(os.path.join(frame_dir, f)).convert('RGB'))[..., ::-1])
    finally:
        writer.release()
    for f in want:
        os.remove(os.path.join(frame_dir, f))
    if not os.listdir(frame_dir):
        os.rmdir(frame_dir)
    return path


def load_label_map(path, size_wh=None):
    """A label map from either kind of file (load_frame_mask), as labels."""
    from utils.utils import colors_to_labels
    m = load_frame_mask(path, size_wh if size_wh is not None else Image.open(path).size)
    return colors_to_labels(m) if m.ndim == 3 else m


class _SizeContext:
    """Everything that depends on the stylised frame size: ring buffers / streams (FramePipeline), the mask plan, the decode
    hook that resizes to the writer size.  One per distinct size met in the clip (normally exactly one)."""

    def __init__(self, args, net, cwct, z_s, s_stats, style_seg, size_wh, writer_wh, device, per_frame=None, mix=None,
                 src_wh=None, segmenter=None, mask_sink=None, matte_hw=None, src_yuv=None, out_yuv=None, style_planes=None,
                 style_meter=None):
        """mix = None (one style, the plain transfer) or (z_s list, style_stats list, style label maps list or None, weights(i),
        alpha_c): every frame is an interpolation with its own weights.  src_wh: --resize device, the frames of this context
        arrive unresized at this size and the pipeline resizes them to size_wh on the card.  matte_hw: --strength_dir, the size
        the frames' mattes arrive at (the stylised size unless the pipeline resizes them on the card).  src_yuv / out_yuv: the
        frames arrive / leave as flat Y'CbCr planes of that YuvSpec (FramePipeline's keywords).  style_planes: --style_map_dir /
        --style_maps_dirs, the shape (P, Hm, Wm) the frames' style planes arrive in; the pipeline makes every frame's map."""
        cw_, ch_ = size_wh
        video_width, video_height = writer_wh
        masked = style_seg is not None
        self.size = size_wh
        plan = None
        zc_shape = (1, 32, ch_, cw_) if net.sp_steps == 2 else (1, 128, ch_ // 2, cw_ // 2)
        # --strength_map: resized to this size and bound once; every frame in flight reads the same rows
        sm = None
        # --strength_labels: the table; the labels are the frame's own (per_frame) or the clip's one map (--content_seg)
        table = static_matte = static_labels = None
        static_map = getattr(args, "strength_map", None)
        if getattr(args, "strength_labels", None) is not None:
            table = cwct.strength_table(args.strength_labels, args.strength_default, device)
            if per_frame is not None:
                if static_map is not None:      # one matte for the clip, times every frame's own label strengths
                    static_matte = torch.from_numpy(load_matte(static_map, size_wh)).to(device)
            else:
                labels = torch.from_numpy(np.ascontiguousarray(load_segment(args.content_seg, size_wh))).to(device)
                if matte_hw is not None:        # every frame's matte, times the clip's label strengths
                    static_labels = labels
                else:                           # nothing changes from frame to frame: the library call, once
                    matte = None if static_map is None else torch.from_numpy(load_matte(static_map, size_wh)).to(device)
                    sm = cwct.frame_strength(zc_shape, matte=matte, labels=labels, table=table)
                    table = None
        elif static_map is not None:
            sm = cwct.bind_strength(load_strength_map(static_map, size_wh, args.mode), zc_shape, device)
        bound = sm
        # --style_map / --style_maps: the planes resized to this size and bound once, like --strength_map; the pipeline hands
        # the bound map to the transform of every frame
        smap = None
        if getattr(args, "style_map_files", None) is not None:
            smap = cwct.bind_style_map(load_style_map(args.style_map_files, size_wh, args.mode), zc_shape, device)
        if per_frame is not None:
            masked = False          # (no static plan: every frame brings its own map)
        if masked:      # one label map for every frame and one style: histograms, uploads and the style side happen once
            content_seg = load_segment(args.content_seg, size_wh)[None, ...]
            with torch.no_grad():
                # (learn_slots: one read-back per size; with at most 8 labels the masked transfer then stays on the packed code)
                if mix is not None:
                    plan = cwct.plan_masks(content_seg, mix[2], zc_shape, [z.shape for z in mix[0]], device)
                    plan = cwct.bind_style(cwct.learn_slots(plan), mix[0])
                else:
                    plan = cwct.bind_style(cwct.learn_slots(cwct.plan_masks(content_seg, style_seg, zc_shape, z_s.shape, device)), z_s)

        def frame_plan(ms, max_slots):       # all of it queued on the frame's stream; buffers belong to the frame's ring slot
            binding, remap = per_frame
            buf = ms.state.get("buffers")
            if buf is None:
                buf = ms.state["buffers"] = cwct.frame_buffers(ch_, cw_, 32, device)
            return cwct.plan_frame(ms.mask, binding, remap=remap, colours=ms.colours, max_slots=max_slots, buffers=buf,
                                   flags=ms.flags)

        def by_label(cs):                    # --stats_by_label: the window of a per-frame plan, its records keyed by label
            return {} if cs is None else dict(content_stats=cs, by_label=True)

        # content_stats: --stats_window, the pipeline's pool over its ring of records (None: the frame's own statistics)
        def transform(z_c, i, ms=None, strength=None, style_map=None, content_stats=None):      # strength: the frame's own map
            sm, cs = strength if strength is not None else bound, content_stats
            if style_map is not None:   # K maps per frame from the styles bound and prefactored once, mixed per row in the decode
                return cwct.transfer_with_stats(z_c, mix[1], mix[4], strength=sm, style_map=style_map, content_stats=cs)
            if mix is not None:         # the mix of THIS frame: one factor launch, styles bound and prefactored
                w, ac = mix[3](i), mix[4]
                if ms is not None:
                    return cwct.transfer_with_plan(z_c, None, frame_plan(ms, 8), alpha_s=w, alpha_c=ac, strength=sm, **by_label(cs))
                if masked:
                    return cwct.transfer_with_plan(z_c, None, plan, alpha_s=w, alpha_c=ac, strength=sm, content_stats=cs)
                return cwct.transfer_with_stats(z_c, mix[1], ac, alpha_s=w, strength=sm, content_stats=cs)
            if ms is not None:
                return cwct.transfer_with_plan(z_c, None, frame_plan(ms, 8), strength=sm, **by_label(cs))
            if args.alpha_c is not None and not masked:     # the style reduced and factored once (s_stats), not per frame
                assert 0.0 <= args.alpha_c <= 1.0
                return cwct.transfer_with_stats(z_c, s_stats, args.alpha_c, strength=sm, content_stats=cs)
            if masked:
                return cwct.transfer_with_plan(z_c, None, plan, strength=sm, content_stats=cs)
            return cwct.transfer_with_stats(z_c, s_stats, strength=sm, content_stats=cs)

        def frame_stats(z_c, out=None):     # the record(s) the transform's route reduces a frame to: the window's ring slots
            return cwct.frame_stats(z_c, plan, out=out)

        decode = None
        lum = bool(getattr(args, "preserve_luminance", False))

        def stylised(z_cs, content_u8):     # the float image at the stylised size: the Lab step comes before the writer's resize
            sty = net(z_cs, forward=False)
            if content_u8 is not None:
                from vstnet_amd.color import luminance_transfer_u8
                sty = luminance_transfer_u8(content_u8, sty, out=sty, to_float=True)
            return sty
        # (with --preserve_luminance the pipeline calls a hook as decode(z_cs, content_u8))
        from vstnet_amd.yuv import DeepYuvSpec
        guided = getattr(args, "upscale", "bicubic") == "guided"
        if guided and (src_wh is None or tuple(src_wh) != (video_width, video_height)):
            raise RuntimeError("--upscale guided writes every frame at the first frame's size (%dx%d) from the source frame on the "
                               "card: a frame of another size, or one outside the device resize's limits, cannot join the clip"
                               % (video_width, video_height))
        if isinstance(out_yuv, DeepYuvSpec) or guided:
            pass        # the pipeline decodes to float planes, blends, resizes (resize_f32; the guided upscale) and converts them
                        # itself: no hook
        elif (cw_, ch_) != (video_width, video_height) and args.resize == 'device':
            from vstnet_amd.resize import resize_to_u8

            # the same resize and quantisation as below, one library call (weights built in double)
            def decode(z_cs, content_u8=None):
                return resize_to_u8(stylised(z_cs, content_u8), (video_height, video_width))
        elif (cw_, ch_) != (video_width, video_height):
            # transforms.Resize((video_height, video_width), BICUBIC) on the float tensor, then quantise
            def decode(z_cs, content_u8=None):
                sty = stylised(z_cs, content_u8)
                sty = F.interpolate(sty, size=(video_height, video_width), mode="bicubic", align_corners=False, antialias=True)
                return sty.mul(255).clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous()
        affinity = bool(getattr(args, "affinity", False))
        if affinity and decode is not None:
            raise RuntimeError("--affinity measures the written frame against the working-size content: a %dx%d frame written at "
                               "%dx%d has no such pair (use --upscale guided, which measures both sizes)"
                               % (cw_, ch_, video_width, video_height))

        def remapped_map(ms):               # what --save_seg_label writes: the frame's map through the plan's remapping table
            if per_frame[1] is None:
                return ms.mask
            from vstnet_amd.masks import apply_lut
            return apply_lut(ms.mask, ms.state["buffers"]["lut"])

        def redo(z_c, i, ms, strength=None):    # more than 8 valid labels: the dense route, cap 32
            sm = strength if strength is not None else bound
            if mix is not None:
                return cwct.transfer_with_plan(z_c, None, frame_plan(ms, 32), alpha_s=mix[3](i), alpha_c=mix[4], strength=sm)
            return cwct.transfer_with_plan(z_c, None, frame_plan(ms, 32), strength=sm)

        self.pipe = FramePipeline(net, transform, ch_, cw_, device=device, depth=args.depth, compute_streams=args.streams,
                                  decode=decode, out_height=video_height, out_width=video_width,
                                  redo=redo if per_frame is not None else None, preserve_luminance=lum, segmenter=segmenter,
                                  seg_work_size=args.seg_size if segmenter is not None else None,
                                  seg_window=args.seg_window if segmenter is not None else 1, seg_decay=args.seg_decay,
                                  mask_sink=mask_sink, mask_map=remapped_map if mask_sink is not None else None,
                                  strength_table=table, matte_hw=None if matte_hw is None else tuple(matte_hw),
                                  static_matte=static_matte, static_labels=static_labels, style_map=smap,
                                  stats_window=getattr(args, "stats_window", 1), stats_decay=getattr(args, "stats_decay", None) or 1.0,
                                  stats_cut=getattr(args, "stats_cut", None) or 0.0, frame_stats=frame_stats,
                                  map_drift=bool(getattr(args, "map_drift", False)),
                                  stats_by_label=bool(getattr(args, "stats_by_label", False)),
                                  **({} if style_planes is None else dict(style_planes=style_planes[0],
                                                                          style_hw=tuple(style_planes[1:]))),
                                  **({} if src_yuv is None else dict(src_yuv=src_yuv)),
                                  **({} if out_yuv is None else dict(out_yuv=out_yuv)),
                                  **({} if not guided else dict(upscale="guided", upscale_radius=args.upscale_radius,
                                                                upscale_eps=args.upscale_eps)),
                                  **({} if not affinity else dict(affinity=True, affinity_radius=args.affinity_radius,
                                                                  affinity_eps=args.affinity_eps)),
                                  **({} if style_meter is None else dict(style_loss=style_meter,
                                                                          content_loss=bool(args.content_loss))),
                                  **({} if not getattr(args, "temporal", False) else dict(temporal=True)),
                                  **({} if getattr(args, "stabilise", None) is None else dict(stabilise=dict(
                                      gain=args.stabilise, sigma=args.stabilise_sigma, limit=args.stabilise_limit))),
                                  **({} if not getattr(args, "estimate_flow", False) else dict(
                                      flow="estimate", flow_mask=args.flow_mask,
                                      flow_params=dict(levels=args.flow_levels, iters=args.flow_iters, radius=args.flow_radius,
                                                       lam=args.flow_lambda))),
                                  **({} if src_wh is None else dict(src_height=src_wh[1], src_width=src_wh[0],
                                                                    max_size=args.max_size, down_scale=net.down_scale,
                                                                    src_deep_resize=isinstance(src_yuv, DeepYuvSpec))))


def _deep_pix_fmt(fmt):
    """whether a --pix_fmt / --out_pix_fmt name is a high-bit-depth one (yuv420p10 ...): known from the command line alone"""
    import re
    m = re.search(r"p(\d+)(le|be)?$", fmt or "")
    return bool(m) and int(m.group(1)) > 8


def check_affinity_args(parser, args):
    """--affinity: what the command line alone decides (the output's depth is checked in main, once the clip is known)."""
    if not args.affinity:
        return
    if not 1 <= args.affinity_radius <= 3:
        parser.error("--affinity_radius must be in 1..3")
    if not 0.0 < args.affinity_eps < float("inf"):
        parser.error("--affinity_eps must be above 0 (and finite)")
    if args.stub_stylise:
        parser.error("--affinity is measured on the card: not with --stub_stylise")


def check_temporal_args(parser, args):
    """--temporal: what the command line alone decides, before anything is read (a y4m input's depth and the written size are
    checked in main, once the clip is known)."""
    if not args.temporal:
        for flag in ("flow_dir", "synthetic_motion"):
            if getattr(args, flag) is not None:
                parser.error("--%s belongs to --temporal" % flag)
        if args.flow_negate:
            parser.error("--flow_negate belongs to --temporal --flow_dir")
        if args.estimate_flow or args.flow_mask:
            parser.error("--estimate_flow and --flow_mask belong to --temporal")
        if args.stabilise is not None:
            parser.error("--stabilise belongs to --temporal: it blends along the flows --temporal measures with")
        return
    if args.stabilise is not None:
        if not 0.0 < args.stabilise < 1.0:
            parser.error("--stabilise GAIN must be inside (0, 1)")
        if not 0.0 < args.stabilise_sigma < float("inf"):
            parser.error("--stabilise_sigma must be above 0 (and finite)")
        if not 0.0 <= args.stabilise_limit < float("inf"):
            parser.error("--stabilise_limit must not be negative (and finite)")
        for flag in ("content_seg_dir", "auto_seg"):
            if getattr(args, flag):
                parser.error("--stabilise does not go with --%s: a frame done again on the dense route would leave a stale frame "
                             "in the recursion" % flag)
    if (args.flow_dir is not None) + (args.synthetic_motion is not None) + bool(args.estimate_flow) != 1:
        parser.error("--temporal needs the motion from exactly one source: --flow_dir DIR, --synthetic_motion N or "
                     "--estimate_flow")
    if args.flow_mask and not args.estimate_flow:
        parser.error("--flow_mask checks an estimated flow against its backward twin: it belongs to --estimate_flow")
    if args.estimate_flow:
        if not 1 <= args.flow_levels <= 8:
            parser.error("--flow_levels must be in 1..8")
        if not 1 <= args.flow_iters <= 16:
            parser.error("--flow_iters must be in 1..16")
        if not 1 <= args.flow_radius <= 7:
            parser.error("--flow_radius must be in 1..7")
        if not 0.0 < args.flow_lambda < float("inf"):
            parser.error("--flow_lambda must be above 0 (and finite)")
    if args.shard != "0/1" or args.gpus > 1:
        parser.error("--temporal compares every frame with the one before it: a shard's first frame would need its neighbour's "
                     "output; not with --shard or --gpus N")
    if args.stub_stylise:
        parser.error("--temporal is measured on the card: not with --stub_stylise")
    if args.upscale == 'guided':
        parser.error("--temporal measures the frame at the stylised size, where the flows are: not with --upscale guided")
    from vstnet_amd.rawyuv import parse_pix_fmt
    out_fmt = args.out_pix_fmt or (args.pix_fmt if args.out_format in ('auto', 'yuv') else None)
    try:
        deep = out_fmt is not None and parse_pix_fmt(out_fmt)[1] > 8
    except ValueError:
        deep = False                            # (check_raw_args reports the name)
    if deep:
        parser.error("--temporal measures decoded 8-bit frames: not with a high-bit-depth output (%s)" % out_fmt)
    if args.flow_negate and args.flow_dir is None:
        parser.error("--flow_negate belongs to --flow_dir")
    if args.synthetic_motion is not None:
        if args.synthetic_motion < 2:
            parser.error("--synthetic_motion N makes N frames: at least 2")
        if os.path.isdir(args.video) or not args.video.lower().endswith(IMG_EXT):
            parser.error("--synthetic_motion makes the clip from one image: --video must name a single image file (%s)"
                         % ", ".join(IMG_EXT))
        for flag in ("content_seg", "content_seg_dir", "strength_dir"):
            if getattr(args, flag) is not None:
                parser.error("--synthetic_motion moves the frames, and the maps of --%s would have to move with them: not "
                             "together" % flag)
        if args.motion_level < 0 or args.shift_level < 0 or args.noise_level < 0:
            parser.error("--motion_level, --shift_level and --noise_level must not be negative")


def check_upscale_args(parser, args):
    """--upscale guided: what the command line alone decides (the input's and output's depth and --resize are checked in main,
    once the clip is known: a y4m input puts --resize device in force by itself)."""
    if args.upscale != 'guided':
        return
    if not 1 <= args.upscale_radius <= 8:
        parser.error("--upscale_radius must be in 1..8")
    if not 0.0 < args.upscale_eps < float("inf"):
        parser.error("--upscale_eps must be above 0 (and finite)")
    if args.mode != 'photorealistic':
        parser.error("--upscale guided fits the stylised frame as a locally affine function of the content, which the "
                     "photorealistic model is trained to be and the artistic one is not: not with --mode %s" % args.mode)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    parser = build_parser()
    args = parser.parse_args(argv)
    check_upscale_args(parser, args)
    check_affinity_args(parser, args)
    from vstnet_amd import style_files
    style_files.check_args(parser, args, deep_out=_deep_pix_fmt(args.out_pix_fmt) or (args.out_pix_fmt is None and args.out_format
                                                                                  in ('auto', 'yuv') and _deep_pix_fmt(args.pix_fmt)))
    if args.style_loss:                     # the style's size from the file's header: nothing is decoded, nothing written yet
        from vstnet_amd.resize import img_resize_size as _style_size
        style_wh = _style_size(Image.open((getattr(args, 'styles', None) or [args.style])[0]).size, args.max_size, 4)
        if min(style_wh) < 9:
            parser.error("--style_loss: the style image is %dx%d after the resize, the encoder needs at least 9x9" % tuple(style_wh))
    check_temporal_args(parser, args)
    style_dirs = check_style_map_dir_args(parser, args)   # (first: its exclusions name the flag, whatever the others would say)
    check_seg_args(parser, args)
    check_window_args(parser, args)
    check_stats_args(parser, args)
    check_strength_args(parser, args)
    args.style_map_files = check_style_map_args(parser, args)      # (before check_mix_args fills --alpha_s in)
    per_label = check_mix_args(args)
    os.makedirs(args.out_dir, exist_ok=True)
    name = clip_name(args)
    raw_size = check_raw_args(parser, args)
    fps_given, args.fps = args.fps is not None, 30 if args.fps is None else args.fps
    if raw_size is not None:                # a headerless file: size, format and rate from the command line
        from vstnet_amd.rawyuv import RawYuvClip
        try:
            frames = RawYuvClip(args.video, raw_size[0], raw_size[1], args.pix_fmt, args.fps, args.yuv_siting)
        except ValueError as e:
            parser.error(str(e))
    elif args.synthetic_motion is not None:
        # the still, resized as a frame would be; it stands in for every frame until the clip is made on the card
        frames = [img_resize(Image.open(args.video).convert('RGB'), args.max_size, down_scale=4)] * args.synthetic_motion
    else:
        frames = read_frames(args.video)
    # raw video: a .y4m input brings its size, rate, layout and range in its header; nothing of it is converted on the host
    from vstnet_amd.y4m import Y4MClip, auto_matrix
    from vstnet_amd.yuv import DeepYuvSpec, YuvSpec
    raw_in = raw_size is not None
    y4m_in = isinstance(frames, Y4MClip) or raw_in        # (the frames arrive as flat planes: a .y4m or a raw file)
    raw_out = args.out_format == 'yuv' or args.out_pix_fmt is not None or (raw_in and args.out_format == 'auto')
    y4m_out = (args.out_format == 'y4m' or y4m_in) and not raw_out
    first_size = frames.size if y4m_in else frames[0].size
    if args.style_map_files is not None:    # the planes at the first frame's stylised size: a pixel that no plane covers
        from vstnet_amd.resize import img_resize_size
        check_style_map_planes(parser, args, args.style_map_files, img_resize_size(first_size, args.max_size, 4))
    mask_files = check_mask_args(args, len(frames))
    matte_files = check_strength_dir(parser, args, len(frames))
    from vstnet_amd.resize import img_resize_size as _sty_size
    plane_files = check_style_map_dirs(parser, args, style_dirs, len(frames), _sty_size(first_size, args.max_size, 4))
    video_width, video_height = writer_size(first_size if y4m_in else frames[0], args.max_size)
    if args.upscale == 'guided':            # the frame is written at the source frame's size
        from vstnet_amd.resize import img_resize_size
        if tuple(first_size) == tuple(img_resize_size(first_size, args.max_size, 4)):
            print("--upscale guided: a %dx%d frame is stylised at its own size, there is nothing to upscale: the plain path "
                  "(--upscale bicubic) is in force" % (first_size[0], first_size[1]), file=sys.stderr)
            args.upscale = 'bicubic'
        else:
            video_width, video_height = int(first_size[0]), int(first_size[1])
    in_spec = out_spec = None
    deep_resize = False
    out_fps = args.fps
    if y4m_in:
        from vstnet_amd.resize import device_supported
        in_spec = out_spec = frames.spec(args.yuv_matrix, args.yuv_range)
        if not fps_given:
            out_fps = frames.fps
        if len(frames) == 0:
            parser.error("%s holds no frame" % args.video)
        deep_in = isinstance(in_spec, DeepYuvSpec)
        if deep_in:                         # the frame enters the encoder as it is, or through the float resize on the card
            from vstnet_amd.resize import MAX_SHRINK, img_resize_size
            deep_resize = img_resize_size(first_size, args.max_size, 4) != tuple(first_size)
            if deep_resize and args.resize != 'device':
                parser.error("a %dx%d %s frame does not pass the resize rule unchanged: with --resize host a high-bit-depth input "
                             "needs its long edge at most --max_size (%d) and both edges multiples of 4; the host float resize "
                             "ahead of the encoder is not built yet: --resize device resizes the planes on the card"
                             % (first_size[0], first_size[1], args.pix_fmt, args.max_size))
            if deep_resize and not device_supported(first_size, args.max_size, 4):
                parser.error("a %dx%d %s frame to --max_size %d is outside the float resize's limits (a step may shrink an axis "
                             "by a factor of %d at the most), and a high-bit-depth input has no host resize"
                             % (first_size[0], first_size[1], args.pix_fmt, args.max_size, MAX_SHRINK))
            if y4m_out:
                parser.error("high-bit-depth output is always a raw .yuv file, never a y4m (--out_format yuv, or --out_pix_fmt "
                             "yuv420p for an 8-bit y4m)")
        elif not device_supported(first_size, args.max_size, 4):
            parser.error("a %dx%d y4m frame to --max_size %d is outside the device resize's limits (a shrink of more than 16x per "
                         "axis), and a y4m input is resized on the card only" % (first_size[0], first_size[1], args.max_size))
        if args.resize == 'host' and not deep_in:
            print("a y4m input is resized on the card: --resize device is in force", file=sys.stderr)
            args.resize = 'device'
        if y4m_out and in_spec.layout == "422":
            parser.error("a y4m output has no 4:2:2 layout here: --out_format yuv")
    elif y4m_out:
        out_spec = YuvSpec("420jpeg", auto_matrix(video_width, video_height) if args.yuv_matrix == 'auto' else args.yuv_matrix,
                           'limited' if args.yuv_range == 'auto' else args.yuv_range)
    deep_in = isinstance(in_spec, DeepYuvSpec)
    deep_resize = deep_in and deep_resize       # a deep frame at its own size: --resize device, the float resize on the card
    out_fmt = None
    if raw_out:         # a raw file at --out_pix_fmt, else in the input's format, else yuv420p; matrix and range: the input's
        from vstnet_amd.rawyuv import pix_fmt_spec
        out_fmt = args.out_pix_fmt or (args.pix_fmt if raw_in else "yuv420p")
        siting = args.yuv_siting if in_spec is None or raw_in or in_spec.layout != "420jpeg" else "centre"
        out_spec = pix_fmt_spec(out_fmt, (video_width, video_height), in_spec.matrix if in_spec is not None else args.yuv_matrix,
                                in_spec.range if in_spec is not None else args.yuv_range, siting)
    deep_out = isinstance(out_spec, DeepYuvSpec)
    if args.upscale == 'guided':
        if deep_in or deep_out:
            parser.error("--upscale guided works on 8-bit frames: not with a high-bit-depth input or output (--pix_fmt / "
                         "--out_pix_fmt above 8 bits)")
        if args.resize != 'device':
            parser.error("--upscale guided needs the source frame on the card: --resize device")
        if args.stub_stylise:
            parser.error("--upscale guided is a step on the card: not with --stub_stylise")
    if args.affinity and deep_out:
        parser.error("--affinity measures a float frame of the guided route or a written 8-bit frame: not with a high-bit-depth "
                     "output (--out_pix_fmt above 8 bits)")
    if args.style_loss:
        from vstnet_amd.resize import img_resize_size
        if deep_out:
            parser.error("--style_loss measures the written 8-bit frame: not with a high-bit-depth output")
        sty_wh = tuple(img_resize_size(first_size, args.max_size, 4))
        if args.content_loss and sty_wh != (video_width, video_height):
            parser.error("--content_loss compares the written frame with its content at the stylised size: a %dx%d frame is "
                         "stylised at %dx%d and written at %dx%d (choose --max_size so that the two agree)"
                         % (first_size[0], first_size[1], sty_wh[0], sty_wh[1], video_width, video_height))
        if min(video_width, video_height) < 9:
            parser.error("--style_loss needs written frames of at least 9x9")
    flow_files = None
    if args.temporal:
        from vstnet_amd.resize import img_resize_size
        if deep_out:
            parser.error("--temporal measures decoded 8-bit frames: not with a high-bit-depth output")
        sty_wh = tuple(img_resize_size(first_size, args.max_size, 4))
        if sty_wh != (video_width, video_height):
            parser.error("--temporal measures the frame at the stylised size, where the flows are: a %dx%d frame is stylised at "
                         "%dx%d and written at %dx%d (choose --max_size so that the two agree)"
                         % (first_size[0], first_size[1], sty_wh[0], sty_wh[1], video_width, video_height))
        if args.flow_dir is not None:
            from vstnet_amd.flowfiles import list_flows
            try:
                flow_files = list_flows(args.flow_dir, len(frames))
            except ValueError as e:
                parser.error(str(e))
    y4m_path = os.path.join(args.out_dir, name + (".y4m" if not raw_out else "_%dx%d_%s.yuv" % (video_width, video_height, out_fmt)))

    if args.gpus > 1:                                   # parent of a multi-GPU run: never initialises a GPU itself
        rc = launch_shards(args, argv)
        if rc != 0:
            raise SystemExit(rc)
        if raw_out:
            from vstnet_amd.rawyuv import merge_parts
            out = merge_parts(y4m_path, [os.path.join(args.out_dir, name, "part_%d.yuv" % r) for r in range(args.gpus)], len(frames),
                              out_spec.frame_bytes(video_height, video_width))
        elif y4m_out:
            from vstnet_amd.y4m import merge_parts
            out = merge_parts(y4m_path, [os.path.join(args.out_dir, name, "part_%d.yuv" % r) for r in range(args.gpus)], len(frames),
                              video_width, video_height, out_fps, out_spec)
        else:
            out = merge_outputs(os.path.join(args.out_dir, name), len(frames), args.out_dir, name, args.fps, (video_width, video_height))
        if args.affinity:                   # the children's parts, in frame order, into the file one process writes
            from vstnet_amd import affinity as aff_files
            joined = aff_files.join_parts([os.path.join(args.out_dir, name, aff_files.part_name(r)) for r in range(args.gpus)],
                                          os.path.join(args.out_dir, name, aff_files.CSV_NAME), len(frames))
            print(aff_files.summary(aff_files.read_csv(joined)))
        if args.style_loss:                 # likewise
            joined = style_files.join_parts([os.path.join(args.out_dir, name, style_files.part_name(r)) for r in range(args.gpus)],
                                            os.path.join(args.out_dir, name, style_files.CSV_NAME), len(frames))
            print(style_files.summary(style_files.read_csv(joined)))
        print("Save stylized video at %s" % out)
        return out

    rank, world = (int(v) for v in args.shard.split("/"))
    lo, hi = shard_range(len(frames), rank, world)
    down_scale = 4
    net = cwct = z_s = s_stats = style_seg = device = None
    masked = args.auto_seg or ((args.content_seg is not None or mask_files is not None) and args.style_seg is not None)
    segmenter = None
    per_frame = host_remap = None
    LAST_RUN.clear()
    LAST_RUN.update(masks={}, redo=0, weights={}, mattes={}, style_maps={})
    affinity = {}                               # --affinity: frame index -> (loss_work[, loss_full])
    style_values, style_meter = {}, None        # --style_loss: frame index -> (loss_s[, loss_c]); the style's StyleLoss
    stabilised = {}                             # --stabilise: frame index -> loss_raw, the decoder's pair
    temporal, clip_flows = {}, None             # --temporal: frame index -> (loss_out, loss_in); the synthetic clip's flows
    drifts, cuts, pooled = [], 0, [0, 0]       # (pooled: frames pooled and label records, --stats_by_label)
    n_frames = len(frames)
    # every frame is an interpolation with its own weights: several styles, a cross-fade, or alpha_c per label under masks
    mixing = len(args.styles) > 1 or args.alpha_s_end is not None or (masked and per_label)
    mix = None

    def weights(i):
        w = LAST_RUN["weights"][i] = mix_weights(args, i, n_frames)
        return w
    if mask_files is not None and args.seg_remap:
        from models.segmentation.SegReMapping import SegReMapping
        host_remap = SegReMapping(args.label_mapping, args.min_ratio)
    if not args.stub_stylise:
        device = torch.device("cuda")
        net = build_network(args.mode, args.ckpoint, args.synthetic_weights, device, args.precision)
        down_scale = net.down_scale
        from models.cWCT import cWCT
        cwct = cWCT(precision=args.precision)
        style = img_resize(Image.open(args.style).convert('RGB'), args.max_size, down_scale=down_scale)
        with torch.no_grad():
            z_s = net.forward_u8(to_tensor_u8(style).to(device))
            s_stats = cwct.style_stats(z_s) if not masked else None
        if args.style_loss:                 # the (first) style's four records, once; every ring slot gets a clone
            from vstnet_amd.vgg import StyleLoss, VGGEncoder        # (the style's size was checked with the flags)
            style_meter = StyleLoss(VGGEncoder(style_files.load_weights(args), device), to_tensor_u8(style).to(device))
        if args.auto_seg:                   # the style is segmented (and self-remapped) once, every frame on its own stream
            check_seg_pixels(args.seg_size, [style.size, (video_width, video_height)])
            segmenter = build_segmenter(args, device)
            seg_remap = device_remapper(args)
            with torch.no_grad():
                s_map = segment_image(segmenter, style, args.seg_size, device)
                if seg_remap is not None:
                    s_map = seg_remap.self_remapping(s_map)
                style_seg = s_map.cpu().numpy()[None, ...]
                per_frame = (cwct.bind_style_labels(z_s, style_seg), seg_remap)
            if rank == 0:
                save_seg_maps(args, {"style_seg": style_seg[0]}, args.out_dir)
        elif mask_files is not None:
            style_seg = load_label_map(args.style_seg, style.size)[None, ...]
        else:
            style_seg = load_segment(args.style_seg, style.size)[None, ...] if masked else None
        if mixing:
            imgs = [style] + [img_resize(Image.open(f).convert('RGB'), args.max_size, down_scale=down_scale)
                              for f in args.styles[1:]]
            with torch.no_grad():
                z_ss = [z_s] + [net.forward_u8(to_tensor_u8(im).to(device)) for im in imgs[1:]]
                stats_all = [cwct.style_stats(z) for z in z_ss] if not masked else None
            segs = None
            if masked:
                load_seg = load_label_map if mask_files is not None else load_segment
                segs = [style_seg] + [load_seg(f, im.size)[None, ...] for f, im in zip(args.style_segs[1:], imgs[1:])]
            # (masks without --interpolate_labels: alpha_c stays ignored, as the reference does)
            mix = (z_ss, stats_all, segs, weights, args.alpha_c if args.alpha_c is not None and (not masked or per_label) else 0.0)
        if mask_files is not None:          # the style side keyed by label, once per clip whatever the frames' maps do
            from vstnet_amd.masks import DeviceSegReMapping
            if host_remap is not None:      # (once per clip: the host class)
                style_seg = host_remap.self_remapping(style_seg[0])[None, ...]
                if mix is not None:
                    mix[2][:] = [style_seg] + [host_remap.self_remapping(sg[0])[None, ...] for sg in mix[2][1:]]
            with torch.no_grad():
                per_frame = (cwct.bind_style_labels(mix[0], mix[2]) if mix is not None else cwct.bind_style_labels(z_s, style_seg),
                             DeviceSegReMapping(host_remap.label_mapping, args.min_ratio) if host_remap is not None else None)

    if args.synthetic_motion is not None:       # the clip with known motion, made on the card from the resized still
        from vstnet_amd.temporal import synthetic_clip
        still = np.asarray(frames[0], dtype=np.uint8)
        cell = min(100, still.shape[0], still.shape[1])     # the reference's 100-pixel cells and blur, as far as the frame has them
        clip, clip_flows, clip_loss_in = synthetic_clip(still, args.synthetic_motion, args.motion_seed, args.motion_level,
                                                        args.shift_level, args.noise_level, device, cell=cell, ksize=cell)
        frames = [Image.fromarray(f) for f in clip.cpu().numpy()]
        LAST_RUN["synthetic"] = dict(frames=clip, flows=clip_flows, loss_in=clip_loss_in)

    writer, frame_dir = None, None
    cv2 = y4m_writer = None
    if y4m_out or raw_out:              # one file, or this shard's headerless part for the parent (or merge_parts by hand)
        from vstnet_amd.y4m import Y4MWriter
        from vstnet_amd.rawyuv import RawYuvWriter
        if world > 1:
            os.makedirs(os.path.join(args.out_dir, name), exist_ok=True)
            y4m_path = os.path.join(args.out_dir, name, "part_%d.yuv" % rank)
        y4m_writer = (RawYuvWriter(y4m_path) if raw_out
                      else Y4MWriter(y4m_path, video_width, video_height, out_fps, out_spec, header=world == 1))
    elif not args.frames_only:
        try:
            import cv2
        except ImportError:
            cv2 = None
    if y4m_writer is not None:
        pass
    elif cv2 is not None:
        writer = cv2.VideoWriter(os.path.join(args.out_dir, name + (".mp4" if world == 1 else "_%d.mp4" % rank)),
                                 cv2.VideoWriter_fourcc('m', 'p', '4', 'v'), args.fps, (video_width, video_height))
    else:
        frame_dir = os.path.join(args.out_dir, name)
        os.makedirs(frame_dir, exist_ok=True)

    dec_workers, enc_workers = host_workers(args.workers)

    def write(i, out):
        if y4m_writer is not None:      # (the flat planes, as the pipeline's out_yuv delivers them)
            y4m_writer.write(out)
        elif writer is not None:
            writer.write(out[..., ::-1])
        else:
            save_png(os.path.join(frame_dir, "%05d.png" % i), out, args.png_level)

    device_resize = args.resize == 'device' and not args.stub_stylise      # (the stub rehearses the flag on the host resize)
    warned = []

    def on_device(size_wh):
        """--resize device: whether a frame of this size is resized on the card (one stderr line for a clip that is not)."""
        from vstnet_amd.resize import device_supported
        if device_supported(size_wh, args.max_size, down_scale):
            return True
        if not warned:
            warned.append(size_wh)
            print("--resize device: a %dx%d frame to --max_size %d is outside the device resize's limits (a shrink of more than "
                  "16x); such frames are resized on the host" % (size_wh[0], size_wh[1], args.max_size), file=sys.stderr)
        return False

    def load_matte_of(i, size_wh, on_card):
        """Frame i's matte: at its own size when the card resizes it, else PIL-BILINEAR-resized to the stylised size here."""
        from vstnet_amd.resize import grey_device_supported
        LAST_RUN["mattes"][i] = matte_files[i]
        m = load_matte(matte_files[i])
        if m.shape == (size_wh[1], size_wh[0]):
            return m
        if on_card and grey_device_supported(m.shape, (size_wh[1], size_wh[0])):
            return m
        if on_card and not matte_warned:
            matte_warned.append(m.shape)
            print("--resize device: a %dx%d matte to %dx%d is outside the device resize's limits (a shrink of more than 16x); "
                  "such mattes are resized on the host" % (m.shape[1], m.shape[0], size_wh[0], size_wh[1]), file=sys.stderr)
        return load_matte(matte_files[i], size_wh)

    matte_warned = []

    def load_planes_of(i, size_wh, on_card):
        """Frame i's style planes, uint8 [P,h,w]: at their own size when the card resizes them, else PIL-BILINEAR-resized to the
        stylised size here (load_matte_of's rule).  The planes of one frame have one size."""
        from vstnet_amd.resize import grey_device_supported
        paths = [names[i] for names in plane_files]
        LAST_RUN["style_maps"][i] = paths
        planes = [load_matte(f) for f in paths]
        for f, m in zip(paths[1:], planes[1:]):
            if m.shape != planes[0].shape:
                raise StylePlanesError("frame %d: the planes of one frame's style map have one size, but %s is %dx%d and %s is %dx%d"
                                       % (i, paths[0], planes[0].shape[1], planes[0].shape[0], f, m.shape[1], m.shape[0]))
        shape = planes[0].shape
        if shape != (size_wh[1], size_wh[0]) and not (on_card and grey_device_supported(shape, (size_wh[1], size_wh[0]))):
            if on_card and not planes_warned:
                planes_warned.append(shape)
                print("--resize device: a %dx%d style plane to %dx%d is outside the device resize's limits (a shrink of more than "
                      "16x); such planes are resized on the host" % (shape[1], shape[0], size_wh[0], size_wh[1]), file=sys.stderr)
            planes = [load_matte(f, size_wh) for f in paths]
        return np.stack(planes)

    planes_warned = []

    def load(i, warm=False):         # decode + resize; EVERY frame is resized on its own (video_transfer.py:161)
        img = frames[i]
        if deep_in and args.stub_stylise:                     # (the rehearsal converts on the host, in numpy: the 8-bit twin)
            from vstnet_amd.yuv import yuv16_to_rgb_host
            img = Image.fromarray(yuv16_to_rgb_host(img, first_size[1], first_size[0], in_spec)[1])
        elif y4m_in and args.stub_stylise:
            from vstnet_amd.yuv import yuv_to_rgb_host
            img = Image.fromarray(yuv_to_rgb_host(img, first_size[1], first_size[0], in_spec))
        if deep_in and not args.stub_stylise:                 # the frame's bytes as read: at the stylised size already, or
            from vstnet_amd.resize import img_resize_size     # (deep_resize) at its own, for the frame's stream to resize
            arr, size_wh = img, img_resize_size(first_size, args.max_size, down_scale) if deep_resize else None
        elif y4m_in and not args.stub_stylise:                # the flat planes as read: the frame's stream converts and resizes
            from vstnet_amd.resize import img_resize_size
            arr, size_wh = img, img_resize_size(first_size, args.max_size, down_scale)
        elif device_resize and args.synthetic_motion is None and on_device(img.size):  # decode only: the frame's stream resizes it
            # (a synthetic clip is made at the stylised size: its frames pass the host rule below unchanged)
            from vstnet_amd.resize import img_resize_size
            arr = np.asarray(img, dtype=np.uint8)
            size_wh = img_resize_size(img.size, args.max_size, down_scale)
        else:
            arr = np.asarray(img_resize(img, args.max_size, down_scale=down_scale), dtype=np.uint8)
            size_wh = None
        sty_wh = size_wh or (tuple(first_size) if arr.ndim == 1 else (arr.shape[1], arr.shape[0]))   # (flat: a deep frame)
        matte = load_matte_of(i, sty_wh, size_wh is not None) if matte_files is not None and not warm else None
        planes = load_planes_of(i, sty_wh, size_wh is not None) if plane_files is not None and not warm else None
        if mask_files is None:
            return i, arr, None, size_wh, matte, planes
        if not warm:                 # (the record lists the maps of the frames this process writes, not its warm-up frames')
            LAST_RUN["masks"][i] = mask_files[i]
        return i, arr, load_frame_mask(mask_files[i], sty_wh), size_wh, matte, planes

    def source():        # background threads, frames in order
        return parallel_map(load, range(lo, hi), workers=dec_workers if isinstance(frames, FrameDir) else 1, ahead=args.depth)

    # numbered PNGs are independent files: encode them on several threads; a video writer takes its frames in order from one
    sink = AsyncSink(write, ahead=2 * enc_workers, workers=1 if writer is not None or y4m_writer is not None else enc_workers)
    seg_sink = seg_writer = flicker = None
    if args.auto_seg and (args.save_seg_label or args.save_seg_color):
        # one remapped map per frame under out_dir/segmentation/ (%05d_label.png, %05d_color.png); a shard writes its own frames
        seg_writer = AsyncSink(lambda i, m: save_seg_maps(args, {"%05d" % i: m}, args.out_dir, quiet=True), ahead=2 * enc_workers,
                               workers=enc_workers)
        flicker = FlickerMeter()

        def seg_sink(i, m):             # (the pipeline calls it in frame order, the writers take the maps in any order)
            flicker(m)
            seg_writer(i, m)
    try:
        if args.stub_stylise:       # host-logic rehearsal: the "stylised" frame is the resized frame at the writer size
            stub_style_seg = None
            if mask_files is not None:
                stub_style_seg = load_label_map(args.style_seg)
                if host_remap is not None:
                    stub_style_seg = host_remap.self_remapping(stub_style_seg)
            for item in source():
                i, arr = item[0], item[1]
                if mixing:
                    weights(i)
                if mask_files is not None:      # what the device does with the map, on the host: it must be a usable map
                    from utils.utils import colors_to_labels
                    seg = colors_to_labels(item[2]) if item[2].ndim == 3 else item[2]
                    if host_remap is not None:
                        seg = host_remap.cross_remapping(host_remap.self_remapping(seg), stub_style_seg)
                    assert seg.shape == arr.shape[:2] and seg.dtype == np.uint8
                out = np.asarray(Image.fromarray(arr).resize((video_width, video_height), Image.BICUBIC))
                if deep_out and deep_resize:    # the float resize ahead of the encoder, then the one to the written size
                    from vstnet_amd.resize import img_resize_float, resize_float
                    from vstnet_amd.yuv import rgb_to_yuv16_host, yuv16_to_rgb_float
                    x = np.clip(img_resize_float(yuv16_to_rgb_float(frames[i], first_size[1], first_size[0], in_spec),
                                                 args.max_size, down_scale), 0.0, 1.0)
                    out = rgb_to_yuv16_host(resize_float(x, (video_height, video_width)), out_spec)
                elif deep_out:          # (a conforming deep input is not resized: its float planes go straight to the other side)
                    from vstnet_amd.yuv import rgb_to_yuv16_host, yuv16_to_rgb_host
                    out = rgb_to_yuv16_host(yuv16_to_rgb_host(frames[i], first_size[1], first_size[0], in_spec)[0] if deep_in
                                            else out / 255.0, out_spec)
                elif y4m_out or raw_out:
                    from vstnet_amd.yuv import rgb_to_yuv_host
                    out = rgb_to_yuv_host(out, out_spec)
                sink(i, out)
        else:
            # consecutive frames of one size stream through that size's pipeline; a size change (rare: the reference resizes
            # every frame on its own, :161) drains it and switches to the other size's context
            contexts = {}
            it = iter(prefetch(source(), ahead=args.depth))
            pending = next(it, None)
            while pending is not None:
                # (pending[3]: the stylised size of a frame that arrives unresized, --resize device; else None)
                # (pending[4]: the frame's matte, --strength_dir; mattes of another size get a context of their own)
                # (pending[5]: the frame's style planes, --style_map_dir / --style_maps_dirs, [P,h,w]; likewise)
                def src_of(item):       # the size a frame arrives at (a y4m frame: flat planes of the header's size)
                    return first_size if item[1].ndim == 1 else (item[1].shape[1], item[1].shape[0])

                def key_of(item):
                    return src_of(item), item[3], None if item[4] is None else item[4].shape, None if item[5] is None else item[5].shape
                key, start = key_of(pending), pending[0]

                run_masks, run_mattes, run_planes = [], [], []       # the maps of the frames the pipeline has taken, in step with them
                run_index = []                       # --temporal: their indices

                def same_size_run():
                    nonlocal pending
                    while pending is not None and key_of(pending) == key:
                        arr = pending[1]
                        run_index.append(pending[0])
                        if mask_files is not None:
                            run_masks.append(pending[2])
                        if matte_files is not None:
                            run_mattes.append(pending[4])
                        if plane_files is not None:
                            run_planes.append(pending[5])
                        pending = next(it, None)
                        yield arr

                def same_size_masks():
                    while True:
                        yield run_masks.pop(0)

                def same_size_mattes():
                    while True:
                        yield run_mattes.pop(0)

                def same_size_planes():
                    while True:
                        yield run_planes.pop(0)

                def same_size_flows():      # frame i's flow maps frame i - 1 onto it: file i - 1, or the clip's own flows[i]
                    sty = key[1] or key[0]
                    while True:
                        i = run_index.pop(0)
                        if i == 0:
                            yield None
                        elif clip_flows is not None:
                            yield clip_flows[i]
                        else:
                            from vstnet_amd.flowfiles import read_flow
                            yield read_flow(flow_files[i - 1], (sty[1], sty[0]), args.flow_negate)
                ctx = contexts.get(key)
                if ctx is None:
                    ctx = contexts[key] = _SizeContext(args, net, cwct, z_s, s_stats, style_seg, key[1] or key[0],
                                                       (video_width, video_height), device, per_frame=per_frame, mix=mix,
                                                       src_wh=key[0] if key[1] is not None else None, segmenter=segmenter,
                                                       mask_sink=seg_sink, matte_hw=key[2], src_yuv=in_spec, out_yuv=out_spec,
                                                       style_planes=key[3], style_meter=style_meter)
                before = ctx.pipe.redo_count
                # a shard's first run also segments the frames just before it, as far as they are of its first frame's size (a
                # size change starts the window over, in one process as in a shard)
                # (--stats_by_label: the two windows add up, and under --content_seg_dir the warm-up frames bring their maps)
                warm, warm_masks = [], []
                if start == lo:
                    for item in (load(j, warm=True) for j in reversed(warmup_frames(lo, args.seg_window, args.stats_window))):
                        if (src_of(item), item[3]) != key[:2]:
                            break
                        warm.insert(0, item[1])
                        warm_masks.insert(0, item[2])
                keyed = args.stats_by_label and mask_files is not None
                try:
                    ctx.pipe.run(same_size_run(), sink, start_index=start, masks=same_size_masks() if mask_files is not None else None,
                                 warmup=warm, mattes=same_size_mattes() if matte_files is not None else None,
                                 **(dict(warmup_masks=warm_masks) if keyed else {}),
                                 **(dict(flows=same_size_flows()) if args.temporal and not args.estimate_flow else {}),
                                 **(dict(style_maps=same_size_planes()) if plane_files is not None else {}))
                except StyleMapZeroSum as e:    # found when the frame retired: the frames before it have been written
                    torch.cuda.synchronize()    # (the frames queued behind it: nothing of them is written)
                    raise SystemExit("frame %d: every plane of its style map is 0 at some pixel, no style would be left there (%s)"
                                     % (e.index, ", ".join(plane_files[d][e.index] for d in range(len(plane_files))))) from None
                LAST_RUN["redo"] += ctx.pipe.redo_count - before
                drifts += list(ctx.pipe.drifts.values())
                if args.affinity:
                    from vstnet_amd.affinity import frame_losses
                    affinity.update({i: frame_losses(v) for i, v in ctx.pipe.affinity.items()})
                if args.style_loss:
                    style_values.update(ctx.pipe.style)
                if args.temporal:
                    temporal.update(ctx.pipe.temporal)
                    stabilised.update(ctx.pipe.stabilised)
                cuts += ctx.pipe.stats_cuts
                pooled[0] += ctx.pipe.pooled_frames
                pooled[1] += ctx.pipe.pooled_labels
    except StylePlanesError as e:       # (raised by a decode worker, re-raised here at its frame's turn)
        raise SystemExit(str(e)) from None
    finally:
        try:
            sink.close()
            if seg_writer is not None:
                seg_writer.close()
        finally:
            if writer is not None:
                writer.release()
                writer = None
            if y4m_writer is not None:
                y4m_writer.close()
    if mask_files is not None or args.auto_seg:
        LAST_RUN["flicker"] = flicker.share if flicker is not None else None
        print("per-frame maps: %d frames, %d done again on the dense route (more than 8 valid labels)%s"
              % (hi - lo, LAST_RUN["redo"], "" if flicker is None else
                 "; %.4f %% of the pixels change label from one frame to the next (mean over %d pairs of saved maps)"
                 % (100 * flicker.share, flicker.pairs)))
    if args.map_drift and not args.stub_stylise:
        LAST_RUN["map_drift"] = float(np.mean(drifts)) if drifts else 0.0
        print("affine map: mean relative change from one frame to the next %.4g (over %d pairs of frames %d..%d, --stats_window %d)"
              % (LAST_RUN["map_drift"], len(drifts), lo, hi - 1, args.stats_window))
    if args.stats_by_label and not args.stub_stylise:
        LAST_RUN["stats_pooled"] = pooled[0] / pooled[1] if pooled[1] else 0.0
        print("statistics window by label: a live label pooled %.3g frames on average (over %d label records of the frames "
              "%d..%d, --stats_window %d)" % (LAST_RUN["stats_pooled"], pooled[1], lo, hi - 1, args.stats_window))
    if args.stats_cut and not args.stub_stylise:
        LAST_RUN["stats_cuts"] = cuts
        print("statistics window: %d of the frames %d..%d had their window cut at the frame before them (--stats_cut %g)"
              % (cuts, lo, hi - 1, args.stats_cut))
    if args.affinity:
        from vstnet_amd import affinity as aff_files
        os.makedirs(os.path.join(args.out_dir, name), exist_ok=True)
        LAST_RUN["affinity"] = dict(affinity)
        LAST_RUN["affinity_csv"] = aff_files.write_csv(
            os.path.join(args.out_dir, name, aff_files.CSV_NAME if world == 1 else aff_files.part_name(rank)), affinity)
        print(aff_files.summary(affinity))
    if args.style_loss:
        os.makedirs(os.path.join(args.out_dir, name), exist_ok=True)
        LAST_RUN["style"] = dict(style_values)
        LAST_RUN["style_csv"] = style_files.write_csv(
            os.path.join(args.out_dir, name, style_files.CSV_NAME if world == 1 else style_files.part_name(rank)), style_values)
        print(style_files.summary(style_values))
    if args.temporal:
        from vstnet_amd import flowfiles
        os.makedirs(os.path.join(args.out_dir, name), exist_ok=True)
        LAST_RUN["temporal"] = dict(temporal)
        LAST_RUN["temporal_csv"] = flowfiles.write_csv(os.path.join(args.out_dir, name, flowfiles.CSV_NAME), temporal, n_frames,
                                                       valid=args.flow_mask)
        print(flowfiles.summary(temporal))
        if args.stabilise is not None:
            rows = {i: (raw, temporal[i][0]) for i, raw in stabilised.items()}
            LAST_RUN["stabilised"] = dict(rows)
            LAST_RUN["stabilise_csv"] = flowfiles.write_stabilise_csv(
                os.path.join(args.out_dir, name, flowfiles.STABILISE_CSV_NAME), rows, n_frames)
            print(flowfiles.stabilise_summary(rows))
    saved = y4m_path if y4m_writer is not None else (frame_dir or args.out_dir)
    print("Save stylized video at %s" % saved)
    return saved


if __name__ == "__main__":
    main()
