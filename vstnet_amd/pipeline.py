"""Overlapped host <-> device frame loop for the video path (replaces the synchronous
per-frame loop of video_transfer.py:186-214).

Frames enter and leave as uint8 HWC in PINNED host ring buffers.  Each frame's H2D copy, encoder pass, cWCT, decoder
pass and D2H copy are queued on one of `compute_streams` HIP streams (consecutive frames alternate, so that the
copies and kernels of two frames overlap on the card); the host only waits when it retires frame i-(depth-1), i.e.
after it has queued `depth-1` newer frames.  A uint8 frame is ~0.1 ms of PCIe time against milliseconds of compute, so
dedicated copy streams (and the cross-stream events they need) would buy nothing.  Nothing here touches
pixels: the output is bit-identical to `net.inverse_u8(transform(net.forward_u8(frame)))` run one frame at a time
(tests/test_gpu_parity.py::test_frame_pipeline_matches_sequential).  `preserve_luminance=True` adds the fork's Lab luminance
blend per frame, one pointwise launch behind the decoder pass on the frame's stream: bit-identical to
`net.inverse_u8(transform(net.forward_u8(frame)), luminance_of=frame)` (tests/test_gpu_luminance.py).

`prefetch()` runs a frame source (decode + resize) in a background thread; PIL and numpy release the GIL in their
inner loops, so decode, the GPU and the sink (encode) overlap.
"""
from __future__ import annotations

import queue
import threading

import numpy as np
import torch


class MaskSlot:
    """A frame's label map while the frame is in flight: `mask` = the uploaded map (uint8 device tensor, [H,W,3] colours or
    [H,W] labels, a view of the ring slot), `colours`, `flags` = the frame's mask flag word (device int32 [1]: VST_MASK_* bits,
    copied back with the frame), `state` = a dict the transform may keep its per-slot buffers in (one tenant at a time)."""

    def __init__(self, index, flags):
        self.index, self.flags, self.state, self.mask, self.colours = index, flags, {}, None, False


class StyleMapZeroSum(ValueError):
    """A frame of a run with style planes has a pixel at which every plane is 0 (raised when the frame retires): `index` is the
    frame's."""

    def __init__(self, index):
        super().__init__(f"frame {index}: every plane of its style map is 0 at some pixel: no style would be left there")
        self.index = index


def logit_ring_slots(window, depth):
    """Buffers in the logit ring of a temporal window of `window` frames with `depth` frames in flight: frame t writes slot
    t % R, and the newest frame that reads what frame t - R left there, t - R + window - 1, must have retired (be at most
    t - depth) by then.  R = window + depth keeps one slot to spare."""
    return int(window) + int(depth)


class WindowRing:
    """The bookkeeping of a ring that lets a frame read what the `window` - 1 frames before it, on other streams, left behind:
    R = logit_ring_slots(window, depth) slots, one "ready" event per slot, the newest frame that reads each slot, and the first
    frame of the run.  It holds no tensors: the logit ring, the record ring and the plan ring are the pipeline's, indexed by
    the slots this class hands out.  A frame calls claim (the slot it is about to write), queues its write, calls publish and
    then gather, all for the stream its work is queued on.

    The ring invariant: slot i % R was written by frame i - R and read by frames i - R .. i - R + W - 1, the newest of which
    is frame i - depth - 1; run() retires frame i - depth (and so every older one) before it submits frame i, and a retired
    frame's stream work is complete, so nothing still reads the slot when frame i overwrites it.  claim asserts that per write
    from what the host knows: the newest reader of the slot and the newest retired frame.  A frame's write is queued ahead of
    its own decoder pass, so the waits of the next frame are as a rule already satisfied.

    new_event() makes an event (torch.cuda.Event in the pipeline); of an event only record(stream) is used, of a stream only
    wait_event(event).  `what` names the ring's contents in the assertion."""

    def __init__(self, window, depth, new_event, what="record"):
        self.window, self.slots, self.what = int(window), logit_ring_slots(window, depth), what
        self.ready = [new_event() for _ in range(self.slots)]
        self.start(0)

    def start(self, first):
        """A run is one window history: it starts at frame `first` (its oldest warm-up frame), and nobody reads anything yet."""
        self.first, self.reader = first, [None] * self.slots

    def claim(self, i, last_retired):
        """The slot frame i is about to write; last_retired: the newest frame the host has retired (None: none yet)."""
        j = i % self.slots
        reader = self.reader[j]
        assert reader is None or (last_retired is not None and reader <= last_retired), \
            f"{self.what} slot {j}: frame {reader} may still read what frame {i} is about to overwrite"
        self.reader[j] = None
        return j

    def publish(self, i, stream):
        """Frame i's write is queued on `stream`: the slot's event behind it."""
        self.ready[i % self.slots].record(stream)

    def gather(self, i, stream):
        """The slots of frame i's window, newest first, its own included: `stream` waits for the older frames' events, and
        frame i becomes their newest reader.  A run's first frames see the frames that exist."""
        ages = min(self.window, i - self.first + 1)
        for a in range(1, ages):
            j = (i - a) % self.slots
            stream.wait_event(self.ready[j])
            self.reader[j] = i
        return [(i - a) % self.slots for a in range(ages)]


def _pinned(shape, dtype):
    """A zeroed pinned host tensor and its numpy view (the two share memory)."""
    t = torch.zeros(shape, dtype=dtype).pin_memory()
    return t, t.numpy()


def _next_entry(it, i, what):
    """The next entry of a per-frame iterable for frame i (None: the run has no such iterable)."""
    if it is None:
        return None
    try:
        return next(it)
    except StopIteration:
        raise ValueError(f"frame {i} has no {what}") from None


class _WindowStats:
    """The `content_stats` of one frame of a statistics window: the frame's own record is already in its ring slot (`held`), and
    the call pools the window's slots, newest first, into the frame ring slot's pooled buffer - on the stream of the transform
    that calls it, behind the waits _stats_window queued there."""

    def __init__(self, pipe, records, k):
        self.pipe, self.records, self.k = pipe, records, k

    def held(self, b):
        return self.records[0]

    def __call__(self, record, b):
        from .cwct import cWCT
        p = self.pipe
        return cWCT.pool_stats(self.records, decay=p.stats_decay, cut=p.stats_cut, out=p.stat_pooled[self.k], used=p.d_used[self.k])


def warmup_counts(seg_window, stats_window, first):
    """(logit-only, statistics) warm-up frames of a run whose first frame is frame `first` of its clip, so that it computes what a
    run over the whole clip computes: the statistics window of frame `first` holds the records of the stats_window - 1 frames
    before it, and the labels of the oldest of those come from the logits of the seg_window - 1 frames before that one.  The
    logit-only frames are the older ones.  Fewer than (seg_window - 1) + (stats_window - 1) frames before `first`: all of them,
    the statistics frames first served."""
    total = min(int(first), (int(seg_window) - 1) + (int(stats_window) - 1))
    n_stats = min(total, int(stats_window) - 1)
    return total - n_stats, n_stats


class _LabelWindowStats:
    """The `content_stats` of one frame of a statistics window by label (cWCT.transfer_with_plan(by_label=True)).  The frame's
    plan is built inside the transform, so everything happens inside the two calls the transfer makes, on its stream:
    record_out offers the frame's record ring slot; the call - handed the record and the frame's plan table - copies the table
    next to the record, records the slot's event, queues the waits on the older slots and pools by label into the frame ring
    slot's pooled buffer (FramePipeline._label_window)."""

    def __init__(self, pipe, i, k, sc):
        self.pipe, self.i, self.k, self.sc = pipe, i, k, sc

    def record_out(self, b):
        return self.pipe._label_slot(self.i)

    def __call__(self, record, b, table):
        return self.pipe._label_window(self.i, self.k, self.sc, record, table)


class FramePipeline:
    def __init__(self, net, transform, height, width, device=None, depth=4, compute_streams=2, decode=None,
                 out_height=None, out_width=None, redo=None, src_height=None, src_width=None, max_size=None, down_scale=4,
                 preserve_luminance=False, segmenter=None, mask_sink=None, mask_map=None, seg_work_size=None, seg_window=1,
                 seg_decay=1.0, strength_table=None, matte_hw=None, static_matte=None, static_labels=None, style_map=None,
                 stats_window=1, stats_decay=1.0, stats_cut=0.0, frame_stats=None, map_drift=False, stats_by_label=False,
                 src_yuv=None, out_yuv=None, src_deep_resize=False, upscale=None, upscale_radius=4, upscale_eps=1e-3,
                 affinity=False, affinity_radius=1, affinity_eps=1e-7, temporal=False, flow=None, flow_mask=False,
                 flow_params=None, style_planes=None, style_hw=None, stabilise=None, style_loss=None, content_loss=False):
        """net: vstnet_amd RevResNet on the GPU; transform(z_c, index) -> z_cs runs on the current stream (cWCT);
        height/width: the (fixed) frame size, multiples of 4; depth: ring slots (>= 2).  decode(z_cs) -> uint8
        [1,out_height,out_width,3] device tensor replaces net.inverse_u8 when the written size differs from the
        stylised size (the reference's writer-size quirk, video_transfer.py:83-86,210-212).
        With run(..., masks=...) the calls are transform(z_c, index, mask_slot) (MaskSlot), and redo(z_c, index, mask_slot)
        -> z_cs is what a frame whose flag word has VST_MASK_OVERFLOW set is done again with when it retires.
        src_height/src_width (with max_size, down_scale): frames arrive at THIS size, unresized; the rings hold source-size
        frames and every frame is resized on the device, on its own stream ahead of the encoder, as
        utils.utils.img_resize(frame, max_size, down_scale) resizes it on the host (vstnet_amd/resize.py: the same bytes);
        height/width must be the size that rule gives.
        preserve_luminance: every frame keeps the Lab luminance of its own content frame (the fork's post-process,
        vstnet_amd/color.py): the default decode is net.inverse_u8(z_cs, luminance_of=<the frame's uint8 device slot>,
        scratch=<the slot's float staging>), and a decode hook is called as decode(z_cs, content_u8) with that slot
        ([1,height,width,3] uint8, valid for the call's stream).
        segmenter: a vstnet_amd.segformer.SegFormer on this device.  Every frame is then segmented on its own stream, from its
        uint8 device slot (after the device resize, if any) straight into the mask ring slot an uploaded map would fill, and the
        calls are transform(z_c, index, mask_slot) as with run(..., masks=...), which it excludes.
        seg_work_size: the segmenter runs on a PIL-exact downscale of the frame with this long edge (SegFormer.work_hw) and its
        logits are sampled at the frame's size (segment_u8's work_size).  The working frame and the resize's pass buffer belong
        to the ring slot; the resize is queued on the frame's stream, ahead of the segmenter and the encoder.
        mask_sink(index, uint8 [H,W] numpy view): called in frame order when a frame with a label map retires, just before its
        sink call, with the map mask_map(mask_slot) gave (a uint8 [H,W] device tensor made on the frame's stream after the
        transform, e.g. the remapped map; default: the slot's own map, which must then be labels, not colours).  The map rides
        back with the frame's D2H copy into a pinned ring of its own.
        seg_window = W > 1 (with a segmenter): a frame's labels come from the weighted mean of the logits of the frame and of the
        W - 1 frames before it (weights segformer.window_weights(frames that exist, seg_decay)); see WindowRing for the ring,
        its invariant and the ordering between the frames' streams.  seg_window = 1 is the per-frame route, with no ring.
        strength_table: float32 [256] (cWCT.strength_table): every frame's strength map is table[label] of the frame's own label
        map - the uploaded map (colours through the dictionary) or the segmenter's, windowed if seg_window says so, always BEFORE
        any remapping: a user names classes of the content.  With run(..., mattes=...) a frame's 8-bit matte scales it (or makes
        the map alone).  The map is made on the frame's stream (cWCT.frame_strength) and transform / redo get one more keyword,
        strength=<the ring slot's StrengthMap>.  matte_hw: the size the mattes arrive at when it is not the frame's; they are
        then resized on the card (resize.resize_grey_u8: PIL's BILINEAR bytes).
        static_matte / static_labels (with a strength_table): uint8 [height,width] device tensors that stand in, for every frame,
        for the side the frames do not bring themselves - one matte for the clip under per-frame labels, or one label map for
        the clip under per-frame mattes.
        style_map: a bound cWCT.StyleMap for this frame size (cWCT.bind_style_map; read-only, shared by the frames in flight):
        transform gets one more keyword, style_map=<it>, for every frame.  Not with masks or a segmenter.
        style_planes = P (with run(..., style_maps=...)): a style map per frame, for regions that move.  Every frame brings P
        8-bit grey planes - P = 1: the weight of the second of two styles, P = 2..8: one plane per style, mixed by v_k / sum_j v_j -
        and its map is made on the frame's stream (cWCT.frame_style_map: one launch, nothing synchronises) into the ring slot's
        StyleMap, which transform gets as style_map=<it>.  style_hw: the size the planes arrive at when it is not the frame's;
        they are then resized on the card, plane by plane (resize.resize_grey_u8: PIL's BILINEAR bytes).  A frame with a pixel
        at which every plane is 0 raises ValueError when it retires (see _style_rings).  It excludes style_map and whatever
        style_map excludes: masks, a segmenter, stats_by_label; it works with whatever style_map works with.
        stats_window = W > 1: a frame's content statistics are pooled with those of the W - 1 frames before it (DESIGN.md section
        5, "Statistics window"; weights stats_decay ** age; stats_cut > 0: a scene cut ends the window, cWCT.pool_stats).
        frame_stats(z_c, out=None) -> the frame's record(s) is the reduction to use - cWCT.frame_stats of the transform's cWCT,
        with its static plan if it has one - and transform gets one more keyword, content_stats=<a callable>, to hand to
        transfer_with_stats / transfer_with_plan.  See WindowRing for the ring, its invariant and the ordering between the
        frames' streams.  Not with a segmenter or run(..., masks=...): their slot sets differ from frame to frame.
        stats_window = 1 is the per-frame route: no ring, no new launch.
        stats_by_label (with stats_window > 1): the window under per-frame label maps - a segmenter or run(..., masks=...), and
        only those.  Records are pooled by the label a slot holds ("Statistics window by label"); transform
        gets content_stats=<a callable> to hand to transfer_with_plan(..., by_label=True) with its plan_frame(..., max_slots <=
        8) plan; frame_stats is not used.  See _label_window.  Not with map_drift: the slot order changes per frame.
        map_drift (any window): the pending affine map(s) of every frame ride back with its D2H copy, and when the frame retires
        the host adds |a_t - a_(t-1)|_2 / |a_t|_2 to `drifts` (per frame index; `mean_drift`).  The transform must return a
        PackedCode with a pending map; a masked one counts the plan's learnt slots.
        src_yuv: a vstnet_amd.yuv.YuvSpec: frames arrive as the flat uint8 planes Y|U|V of a source-size frame (a y4m frame:
        src_yuv.frame_bytes bytes).  The pinned ring and a device ring hold planes; on the frame's stream the planes go up and
        yuv_to_rgb_u8 fills the slot the RGB upload fills otherwise (the source slot under a device resize, else the encoder's
        input), and everything proceeds as with RGB frames: bit-identical to feeding the frames yuv_to_rgb_u8 gives.  The
        planes' slot is reused under the source slot's rule: `consumed[k]` is recorded after the conversion has read it and the
        next tenant's H2D copy waits for the event.  Warm-up frames take the same route.
        out_yuv: a YuvSpec: the uint8 frame the decode (or the decode hook, or a redo) made is converted by rgb_to_yuv_u8 into
        a per-slot flat device buffer, which is what the D2H copy carries; sink gets the flat uint8 view of
        out_yuv.frame_bytes(out_height, out_width) bytes.  Without the two keywords: no new buffer, no new launch.
        Either keyword also takes a vstnet_amd.yuv.DeepYuvSpec (9..16-bit samples), each on its own (DESIGN.md section 6,
        "High-bit-depth edge").  A deep src_yuv: the rings hold the frame's bytes as before; yuv16_to_rgb_f32 fills a per-slot
        fp32 [1,3,H,W] buffer, which is what the encoder reads - net(x), not forward_u8 -, and d_in[k] with the same pixels as
        bytes, which is what a segmenter, the strength labels and the uint8 luminance step go on reading.  The float slot is
        reused under the rule of d_in[k] (`consumed[k]`): the encoder reads it last, or the luminance step when that reads it.
        It excludes src_height / src_width - the frame arrives at the stylised size - unless src_deep_resize=True: then the rings
        hold source-size planes and yuv.DeepImgResize (one per ring slot: img_resize restated in float, DESIGN.md section 6, "Deep
        resize") fills d_xf[k] and d_in[k] at the stylised size on the frame's stream, warm-up frames included; `consumed[k]`
        keeps its rule and everything behind the two slots is unchanged.  A deep out_yuv: the frame is decoded to
        float planes (net._inverse into a per-slot buffer), preserve_luminance blends there (from the float content planes of a
        deep source, else from d_in[k]), resize_f32 takes it to (out_height, out_width) if that differs, and rgb_f32_to_yuv16
        writes the slot's flat device buffer.  It excludes a decode hook.
        upscale="guided" ("Guided upscale"; None or "bicubic": nothing changes): the frame leaves at the
        SOURCE size, made by vstnet_amd.guided.GuidedUpscale (one per ring slot) from the slot's three frames - the resized
        content d_in[k] as the guide, the decoder's float output (after the Lab step of preserve_luminance) as the target, the
        source frame d_src[k] as what the fitted coefficients are applied to; upscale_radius (1..8) and upscale_eps (> 0) are the
        filter's window and ridge.  It needs src_height / src_width with a uint8 source (RGB frames or an 8-bit YuvSpec) and
        (out_height, out_width) == (src_height, src_width); it excludes a decode hook and a deep out_yuv.  An 8-bit out_yuv
        converts the frame as it does any other.  The source slot's last read is then the apply kernel, so `consumed[k]` is
        recorded behind it, not behind the resize.
        affinity=True ("Affinity loss"; off: nothing changes): every frame's Matting-Laplacian loss
        (vstnet_amd.matting, window affinity_radius 1..3, ridge affinity_eps > 0) is queued on the frame's stream behind its
        decode, rides home in a pinned ring and is read when the frame retires: self.affinity[i] is float64 [3], the loss per
        channel at the working size.  Under upscale="guided" that is the decoder's FLOAT frame (after the Lab step, before the
        writer's epilogue) against d_in[k], and three more values follow: the WRITTEN uint8 full-size frame against the source
        frame d_src[k].  Every other route decodes straight to uint8 and the float frame never exists: the decoded uint8 frame
        (before an 8-bit out_yuv converts it) is measured against d_in[k], which needs (out_height, out_width) == (height,
        width).  It excludes a deep out_yuv.  The written bytes are those without the flag.
        temporal=True ("Temporal loss"; off: nothing changes) with run(..., flows=...): every frame that has a
        predecessor and a flow gets two values, the temporal loss (vstnet_amd.temporal: mean |warp(frame i-1, flow i) - frame i|,
        the mean over the three channels) of the DECODED uint8 pair (before any out_yuv conversion) and of the encoder's INPUT
        pair d_in; self.temporal[i] = (loss_out, loss_in) is read when the frame retires.  See _temporal for the history ring,
        its invariant and the ordering between the frames' streams.  It needs (out_height, out_width) == (height, width) and
        excludes a deep out_yuv and upscale='guided'.  The written bytes are those without the flag.
        flow="estimate" (with temporal=True; DESIGN.md section 6, "Optical flow"): run() is called without flows=, and every frame
        with a predecessor gets its flow from the slot's vstnet_amd.flow.FlowEstimator, on the pair of INPUT frames the history
        ring holds; flow_params: a dict of estimate_flow's levels / iters / radius / lam.  flow_mask=True also estimates the flow
        of the swapped pair, takes the forward-backward mask and restricts both losses to its pixels: self.temporal[i] is then
        (loss_out, loss_in, valid_share).
        stabilise=True or dict(gain=, sigma=, limit=) (with temporal=True; DESIGN.md section 6, "Stabiliser"; None: no buffer, no
        event, no launch, every byte and value as before): every frame with a live predecessor and a flow is blended, right behind
        its decode, with the frame WRITTEN before it sampled along the flow (vstnet_amd.stabilise: the weight falls off where the
        input pair changed along that flow; with flow_mask the slot's mask is the kernel's `valid`) into the history ring's third
        plane t_written[k]; that plane is what the affinity loss, an 8-bit out_yuv and the D2H copy read, so the written bytes are
        the stabilised ones, and it is the next frame's prev_written: the filter is recursive.  A frame without a predecessor or
        a flow is copied there as it is.  self.temporal[i][0] is then the loss of the WRITTEN pair, and self.stabilised[i] =
        loss_raw is that of the decoder's pair.  The defaults (gain 0.7, sigma 8, limit 24 levels) are starting values from a
        numpy prototype on constructed clips; picture quality is unmeasured.  It excludes a segmenter and run(..., masks=...): a
        frame done again by _redo would leave a stale frame in the recursion.  See _temporal for the ordering.
        style_loss=<vstnet_amd.vgg.StyleLoss> ("Style loss"; None: no buffer, no event, no launch): every
        frame's loss_s against that object's style - the VGG-19 chain on the uint8 frame the sink receives, so behind the Lab
        step, the guided upscale and the stabiliser's t_written, before an 8-bit out_yuv converts it - is queued on the frame's
        stream, rides home in a pinned ring and is read when the frame retires: self.style[i] = (loss_s,).  Each ring slot has
        a clone of the object (its own workspace; the style's records are shared).  content_loss=True adds loss_c against the
        encoder's input d_in[k]: self.style[i] = (loss_s, loss_c); it needs (out_height, out_width) == (height, width).  A frame
        done again by _redo is measured on its second decode.  It excludes a deep out_yuv.  The written bytes are those without
        the flag."""
        if not torch.cuda.is_available():
            raise RuntimeError("FramePipeline needs the GPU (no CPU fallback)")
        if depth < 2:
            raise ValueError("depth must be >= 2")
        if height % 4 or width % 4 or height < 8 or width < 8:
            raise ValueError(f"frame size must be multiples of 4 and >= 8 (got {height}x{width})")
        self.net, self.transform = net, transform
        self.decode = decode if decode is not None else net.inverse_u8
        self.preserve_luminance, self.custom_decode = bool(preserve_luminance), decode is not None
        self.H, self.W, self.depth = height, width, depth
        self.Ho, self.Wo = out_height or height, out_width or width
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.Hs, self.Ws = (height, width) if src_height is None else (int(src_height), int(src_width))
        self.resizers = self.deep_resizers = None
        from .yuv import DeepYuvSpec
        if src_height is not None and isinstance(src_yuv, DeepYuvSpec):
            # a deep source at its own size: the float restatement of img_resize, fused with the conversion (yuv.DeepImgResize)
            if not src_deep_resize:
                raise ValueError("a high-bit-depth source arrives at the stylised size: the float resize in front of the encoder, "
                                 "the deep edge's follow-up, is opt-in - src_height / src_width go with a DeepYuvSpec only in a "
                                 "pipeline made with src_deep_resize=True, which resizes the planes on the card")
            from .yuv import DeepImgResize
            if src_width is None or max_size is None:
                raise ValueError("src_height needs src_width and max_size")
            # one per ring slot: the pass buffers belong to the frame in flight
            self.deep_resizers = [DeepImgResize((self.Hs, self.Ws), src_yuv, max_size, down_scale, self.device) for _ in range(depth)]
            if self.deep_resizers[0].size_wh != (width, height):
                raise ValueError(f"a {self.Ws}x{self.Hs} frame resizes to {self.deep_resizers[0].size_wh}, not to {width}x{height}")
        elif src_height is not None:
            from .resize import DeviceImgResize
            if src_width is None or max_size is None:
                raise ValueError("src_height needs src_width and max_size")
            # one per ring slot: the pass buffers belong to the frame in flight
            self.resizers = [DeviceImgResize((self.Hs, self.Ws), max_size, down_scale, self.device) for _ in range(depth)]
            if self.resizers[0].size_wh != (width, height):
                raise ValueError(f"a {self.Ws}x{self.Hs} frame resizes to {self.resizers[0].size_wh}, not to {width}x{height}")
        self.src_yuv, self.out_yuv = src_yuv, out_yuv
        self.src_deep = self.out_deep = False
        if upscale not in (None, "bicubic", "guided"):
            raise ValueError(f"upscale must be None, 'bicubic' or 'guided', got {upscale!r}")
        self.upscalers = None
        if upscale == "guided":
            if self.resizers is None:
                raise ValueError("upscale='guided' needs the source frame on the card: src_height / src_width (with max_size) and "
                                 "a uint8 source - RGB frames or an 8-bit YuvSpec, not a high-bit-depth src_yuv")
            if (self.Ho, self.Wo) != (self.Hs, self.Ws):
                raise ValueError(f"upscale='guided' writes the frame at the source size: out_height, out_width must be "
                                 f"{self.Hs}, {self.Ws}, got {self.Ho}, {self.Wo}")
            if decode is not None:
                raise ValueError("a decode hook does not go with upscale='guided': the pipeline decodes to float planes at the "
                                 "working size and upscales them itself")
            if isinstance(out_yuv, DeepYuvSpec):
                raise ValueError("a high-bit-depth out_yuv does not go with upscale='guided': the guided upscale writes uint8 frames")
            from .guided import GuidedUpscale
            # one per ring slot: the coefficient planes and the fit's workspace belong to the frame in flight
            self.upscalers = [GuidedUpscale((height, width), (self.Hs, self.Ws), upscale_radius, upscale_eps, self.device)
                              for _ in range(depth)]
        self.affinity_on = bool(affinity)
        self.affinity = {}                      # frame index -> float64 [3] (working size) or [6] (then the full size)
        self.aff_work = self.aff_full = None
        if self.affinity_on:
            if isinstance(out_yuv, DeepYuvSpec):
                raise ValueError("affinity does not go with a high-bit-depth out_yuv: the loss is taken on the float frame of the "
                                 "guided route or on a written uint8 frame")
            if self.upscalers is None and (self.Ho, self.Wo) != (height, width):
                raise ValueError(f"affinity measures the written frame against the working-size content: out_height, out_width "
                                 f"must be {height}, {width} (got {self.Ho}, {self.Wo}) unless upscale='guided'")
            from .matting import MattingLoss
            # one per ring slot: the workspace belongs to the frame in flight
            self.aff_work = [MattingLoss((height, width), affinity_radius, affinity_eps, self.device) for _ in range(depth)]
            if self.upscalers is not None:
                self.aff_full = [MattingLoss((self.Hs, self.Ws), affinity_radius, affinity_eps, self.device) for _ in range(depth)]
        self.style = {}                         # frame index -> (loss_s,) or (loss_s, loss_c)
        self.style_meters = None
        self.content_loss = bool(content_loss)
        if style_loss is None:
            if self.content_loss:
                raise ValueError("content_loss goes with style_loss: the two share the encoder's run on the written frame")
        else:
            if isinstance(out_yuv, DeepYuvSpec):
                raise ValueError("style_loss does not go with a high-bit-depth out_yuv: the loss is taken on the written uint8 frame")
            if self.content_loss and (self.Ho, self.Wo) != (height, width):
                raise ValueError(f"content_loss compares the written frame with the content at the stylised size: out_height, "
                                 f"out_width must be {height}, {width} (got {self.Ho}, {self.Wo})")
            from .vgg import MIN_EDGE
            if min(self.Ho, self.Wo) < MIN_EDGE:
                raise ValueError(f"style_loss needs written frames of at least {MIN_EDGE} x {MIN_EDGE}, got {self.Ho} x {self.Wo}")
            from .vgg import indexed_device
            if style_loss.device != indexed_device(self.device):
                raise ValueError(f"style_loss is on {style_loss.device}, the pipeline on {self.device}")
            # one per ring slot: the workspace, the records and the relu4_1 maps belong to the frame in flight
            self.style_meters = [style_loss.clone() for _ in range(depth)]
        self.temporal_on = bool(temporal)
        self.temporal = {}                      # frame index -> (loss_out, loss_in), each the mean over the three channels
        if flow not in (None, "estimate"):
            raise ValueError(f"flow must be None or 'estimate', got {flow!r}")
        self.flow_estimate, self.flow_mask = flow == "estimate", bool(flow_mask)
        if self.flow_estimate and not self.temporal_on:
            raise ValueError("flow='estimate' goes with temporal=True: the flow serves the temporal loss alone")
        if (self.flow_mask or flow_params) and not self.flow_estimate:
            raise ValueError("flow_mask and flow_params go with flow='estimate'")
        self.flow_params = dict(flow_params or {})
        if self.temporal_on:
            if isinstance(out_yuv, DeepYuvSpec):
                raise ValueError("temporal does not go with a high-bit-depth out_yuv: the loss is taken on decoded uint8 frames")
            if self.upscalers is not None:
                raise ValueError("temporal does not go with upscale='guided': the flows are at the stylised size, the written "
                                 "frames at the source size")
            if (self.Ho, self.Wo) != (height, width):
                raise ValueError(f"temporal measures the decoded frame under flows at the stylised size: out_height, out_width "
                                 f"must be {height}, {width} (got {self.Ho}, {self.Wo})")
        self.stabilised = {}                    # frame index -> loss_raw: the temporal loss of the decoder's pair (stabilise)
        self.stab_params = None
        if stabilise is not None and stabilise is not False:
            from .stabilise import DEFAULTS as STAB_DEFAULTS, check_params
            if not self.temporal_on:
                raise ValueError("stabilise goes with temporal=True: it blends along the flows and within the history ring the "
                                 "temporal loss keeps")
            if segmenter is not None:
                raise ValueError("stabilise does not go with per-frame mask slots (a segmenter or run(..., masks=...)): a frame "
                                 "done again when it retires would leave a stale frame in the recursion")
            if stabilise is not True and not isinstance(stabilise, dict):
                raise ValueError(f"stabilise must be None, True or a dict of gain / sigma / limit, got {stabilise!r}")
            given = {} if stabilise is True else dict(stabilise)
            if set(given) - set(STAB_DEFAULTS):
                raise ValueError(f"stabilise takes gain, sigma and limit, got {sorted(set(given) - set(STAB_DEFAULTS))}")
            self.stab_params = dict(zip(("gain", "sigma", "limit"), check_params(**{**STAB_DEFAULTS, **given})))
        if src_yuv is not None or out_yuv is not None:
            from .yuv import YuvSpec
            if not all(s is None or isinstance(s, (YuvSpec, DeepYuvSpec)) for s in (src_yuv, out_yuv)):
                raise ValueError("src_yuv / out_yuv are vstnet_amd.yuv YuvSpec or DeepYuvSpec objects")
            self.src_deep, self.out_deep = isinstance(src_yuv, DeepYuvSpec), isinstance(out_yuv, DeepYuvSpec)
            if self.out_deep and decode is not None:
                raise ValueError("a decode hook does not go with a high-bit-depth out_yuv: the pipeline decodes to float planes, "
                                 "resizes them to (out_height, out_width) and converts them itself")
        in_shape = (self.Hs, self.Ws, 3) if src_yuv is None else (src_yuv.frame_bytes(self.Hs, self.Ws),)
        out_shape = (self.Ho, self.Wo, 3) if out_yuv is None else (out_yuv.frame_bytes(self.Ho, self.Wo),)
        self.in_shape = in_shape
        with torch.cuda.device(self.device):
            self.h_in, self.h_in_np = _pinned((depth,) + in_shape, torch.uint8)
            self.h_out, self.h_out_np = _pinned((depth,) + out_shape, torch.uint8)
            # the planes of the frames in flight, as they came (src_yuv) and as they leave (out_yuv): one flat slot per ring slot
            self.d_yuv = torch.empty((depth,) + in_shape, dtype=torch.uint8, device=self.device) if src_yuv is not None else None
            self.d_out_yuv = (torch.empty((depth,) + out_shape, dtype=torch.uint8, device=self.device)
                              if out_yuv is not None else None)
            self.d_in = torch.empty((depth, 1, height, width, 3), dtype=torch.uint8, device=self.device)
            self.d_src = (torch.empty((depth, self.Hs, self.Ws, 3), dtype=torch.uint8, device=self.device)
                          if self.resizers is not None else None)
            # the float planes between the decoder pass and the Lab step: one per ring slot, since the frames in flight are on
            # different streams
            self.lum_scratch = ([torch.empty((1, 3, height, width), dtype=torch.float32, device=self.device) for _ in range(depth)]
                                if self.preserve_luminance and decode is None and not self.out_deep
                                and self.upscalers is None else None)
            # the guided upscale: the decoder's float output at the working size and the frame at the source size, per ring slot
            self.d_up = self.d_up_out = None
            if self.upscalers is not None:
                self.d_up = torch.empty((depth, 1, 3, height, width), dtype=torch.float32, device=self.device)
                self.d_up_out = torch.empty((depth, 1, self.Hs, self.Ws, 3), dtype=torch.uint8, device=self.device)
            # the high-bit-depth edge: the encoder's float input (a deep source) and the decoder's float output, then the same at
            # the written size with the resize's pass buffer (a deep output), one of each per ring slot
            self.d_xf = self.d_of = self.d_of_lum = self.d_of_rs = self.d_of_tmp = None
            if self.src_deep:
                self.d_xf = torch.empty((depth, 1, 3, height, width), dtype=torch.float32, device=self.device)
            if self.out_deep:
                self.d_of = torch.empty((depth, 1, 3, height, width), dtype=torch.float32, device=self.device)
                if self.preserve_luminance and self.src_deep:       # (the float Lab step does not write over its input)
                    self.d_of_lum = torch.empty((depth, 1, 3, height, width), dtype=torch.float32, device=self.device)
                if (self.Ho, self.Wo) != (height, width):
                    self.d_of_rs = torch.empty((depth, 1, 3, self.Ho, self.Wo), dtype=torch.float32, device=self.device)
                    self.d_of_tmp = torch.empty((depth, 3 * height * self.Wo), dtype=torch.float32, device=self.device)
            self.s_comp = [torch.cuda.Stream(device=self.device) for _ in range(max(1, compute_streams))]
            # fp16 modes: the library's range flags travel with every frame (4 words, appended to its D2H copy) and are looked
            # at when the frame is retired - saturation is an error of THAT frame, not a silent clamp somewhere in the clip
            self.d_flags = torch.zeros((depth, 4), dtype=torch.int32, device=self.device)
            self.h_flags, self.h_flags_np = _pinned((depth, 4), torch.int32)
            self.flag_check = [False] * depth
            self.mask_check = [False] * depth
            self.redo = redo
            self.segmenter = segmenter
            self.seg_work = self.seg_tmp = None
            if seg_work_size is not None:
                if segmenter is None:
                    raise ValueError("seg_work_size belongs to a segmenter")
                from .resize import MAX_SHRINK
                hw, ww = segmenter.work_hw(height, width, seg_work_size)
                if height > MAX_SHRINK * hw or width > MAX_SHRINK * ww:
                    raise ValueError(f"seg_work_size {seg_work_size} shrinks a {width}x{height} frame to {ww}x{hw}: more than the "
                                     f"device resize's {MAX_SHRINK}x per axis")
                if (hw, ww) != (height, width):
                    self.seg_work = torch.empty((depth, hw, ww, 3), dtype=torch.uint8, device=self.device)
                    self.seg_tmp = torch.empty((depth, height * ww * 3), dtype=torch.uint8, device=self.device)
            self.seg_window, self.seg_decay = int(seg_window), float(seg_decay)
            self.logit_ring = self.logit_mix = self.logit_window = self.stat_window = self.last_retired = None
            self.warm_slots = set()                 # frame ring slots whose tenant was a warm-up frame: nothing retires those
            if self.seg_window != seg_window or self.seg_window < 1:
                raise ValueError(f"seg_window must be a positive integer, got {seg_window}")
            if self.seg_window > 1:
                self._logit_rings()
            self.mask_sink, self.mask_map = mask_sink, mask_map
            self.h_seg = self.h_seg_np = None
            if mask_sink is not None:
                self.h_seg, self.h_seg_np = _pinned((depth, height, width), torch.uint8)
            self.strength_table = None
            if strength_table is not None:
                t = strength_table if torch.is_tensor(strength_table) else torch.from_numpy(np.asarray(strength_table))
                if t.dtype != torch.float32 or tuple(t.shape) != (256,):
                    raise ValueError("strength_table must be float32 [256] (cWCT.strength_table)")
                self.strength_table = t.to(self.device).contiguous()
            self.matte_hw = (height, width) if matte_hw is None else (int(matte_hw[0]), int(matte_hw[1]))
            if self.matte_hw != (height, width):
                from .resize import grey_device_supported
                if not grey_device_supported(self.matte_hw, (height, width)):
                    raise ValueError(f"mattes of {self.matte_hw[1]}x{self.matte_hw[0]} to {width}x{height} frames are outside the "
                                     "device resize's limits: resize them on the host")
            for name, t in (("static_matte", static_matte), ("static_labels", static_labels)):
                if t is not None and (self.strength_table is None or not torch.is_tensor(t) or t.dtype != torch.uint8
                                      or tuple(t.shape) != (height, width) or not t.is_cuda or not t.is_contiguous()):
                    raise ValueError(f"{name} is a contiguous uint8 [{height},{width}] tensor on {self.device} and needs a "
                                     "strength_table")
            self.static_matte, self.static_labels = static_matte, static_labels
            if style_map is not None:
                from .cwct import StyleMap
                if not isinstance(style_map, StyleMap) or style_map.code_shape[0] != 1 or style_map.rows is None \
                        or style_map.code_shape[2] * style_map.code_shape[3] * style_map.code_shape[1] != 32 * height * width:
                    raise ValueError(f"style_map must be a bound StyleMap (cWCT.bind_style_map) of one {width}x{height} frame's code")
                if segmenter is not None:
                    raise ValueError("style maps are not supported on the masked routes")
            self.style_map = style_map
            self.style_planes, self.style_hw = None, (height, width)
            if style_planes is not None:
                if int(style_planes) != style_planes or not 1 <= int(style_planes) <= 8:
                    raise ValueError(f"style_planes must be an integer in 1..8 (1: the ramp between two styles), got {style_planes}")
                if style_map is not None:
                    raise ValueError("style_planes (a style map per frame) and style_map (one map for the clip) are mutually "
                                     "exclusive")
                if segmenter is not None or stats_by_label:
                    raise ValueError("style maps are not supported on the masked routes: style_planes does not go with a "
                                     "segmenter or stats_by_label (nor with run(..., masks=...))")
                self.style_planes = int(style_planes)
                if style_hw is not None:
                    self.style_hw = (int(style_hw[0]), int(style_hw[1]))
                if self.style_hw != (height, width):
                    from .resize import grey_device_supported
                    if not grey_device_supported(self.style_hw, (height, width)):
                        raise ValueError(f"style planes of {self.style_hw[1]}x{self.style_hw[0]} to {width}x{height} frames are "
                                         "outside the device resize's limits: resize them on the host")
            elif style_hw is not None:
                raise ValueError("style_hw belongs to style_planes")
            self.stats_window, self.stats_decay, self.stats_cut = int(stats_window), float(stats_decay), float(stats_cut)
            if self.stats_window != stats_window or not 1 <= self.stats_window <= 8:
                raise ValueError(f"stats_window must be an integer in 1..8, got {stats_window}")
            if not 0.0 < self.stats_decay <= 1.0:
                raise ValueError(f"stats_decay must be in (0, 1], got {stats_decay}")
            if not 0.0 <= self.stats_cut < float("inf"):
                raise ValueError(f"stats_cut must be >= 0 and finite, got {stats_cut}")
            self.frame_stats = frame_stats
            self.stats_by_label = bool(stats_by_label)
            if self.stats_by_label and self.stats_window == 1:
                raise ValueError("stats_by_label belongs to stats_window W with W > 1")
            if self.stats_by_label and map_drift:
                raise ValueError("map_drift does not go with stats_by_label: the slot order changes from frame to frame")
            if self.stats_by_label and style_map is not None:
                raise ValueError("style maps are not supported on the masked routes")
            if self.stats_window > 1:
                if segmenter is not None and not self.stats_by_label:
                    raise ValueError("stats_window does not go with a segmenter: the label slots differ from frame to frame")
                if frame_stats is None and not self.stats_by_label:
                    raise ValueError("stats_window needs frame_stats (cWCT.frame_stats of the transform's cWCT and plan)")
                self._stat_rings()
            self.map_drift = bool(map_drift)
            self.h_aff = self.h_aff_np = None      # pinned ring of the frames' affine records: made by the first frame
            # affinity: the frames' 3 (working size) or 6 (then the full size) loss values, on the card and in a pinned ring
            self.d_affinity = self.h_affinity = self.h_affinity_np = None
            if self.affinity_on:
                self.n_affinity = 6 if self.aff_full is not None else 3
                self.d_affinity = torch.zeros((depth, self.n_affinity), dtype=torch.float64, device=self.device)
                self.h_affinity, self.h_affinity_np = _pinned((depth, self.n_affinity), torch.float64)
            # style loss: the frames' one or two values, on the card and in a pinned ring
            self.d_style = self.h_style = self.h_style_np = None
            if self.style_meters is not None:
                n_style = 2 if self.content_loss else 1
                self.d_style = torch.zeros((depth, n_style), dtype=torch.float64, device=self.device)
                self.h_style, self.h_style_np = _pinned((depth, n_style), torch.float64)
            # temporal: per ring slot the frame's flow (pinned and on the card), its history - a copy of the encoder's input and
            # of the decoded frame, which outlive the slot's own buffers' reuse rules -, a TemporalLoss and the six values
            self.t_flow_h = self.t_flow_h_np = self.t_flow = self.t_in = self.t_out = self.t_meters = self.t_estimators = None
            self.d_temporal = self.h_temporal = self.h_temporal_np = self.t_written = self.t_blended = None
            if self.temporal_on:
                from .temporal import TemporalLoss
                if self.flow_estimate:              # one per ring slot: workspace, backward flow and mask belong to the slot
                    from .flow import FlowEstimator
                    self.t_estimators = [FlowEstimator((height, width), mask=self.flow_mask, device=self.device,
                                                       **self.flow_params) for _ in range(depth)]
                else:
                    self.t_flow_h, self.t_flow_h_np = _pinned((depth, 2, height, width), torch.float32)
                self.t_flow = torch.empty((depth, 2, height, width), dtype=torch.float32, device=self.device)
                self.t_in = torch.empty((depth, height, width, 3), dtype=torch.uint8, device=self.device)
                self.t_out = torch.empty((depth, height, width, 3), dtype=torch.uint8, device=self.device)
                # one per ring slot: its workspace serves the slot's two calls, which follow one another on the frame's stream
                self.t_meters = [TemporalLoss((height, width), self.device) for _ in range(depth)]
                n_val = 4 if self.flow_mask else 3  # with the mask: the three means and the share of valid pixels
                n_row = 3 if self.stab_params is not None else 2    # stabilise: the decoder's pair is measured too
                self.d_temporal = torch.zeros((depth, n_row, n_val), dtype=torch.float64, device=self.device)
                self.h_temporal, self.h_temporal_np = _pinned((depth, n_row, n_val), torch.float64)
                self.t_ready = [torch.cuda.Event() for _ in range(depth)]      # the slot's history has been written
                self.t_read = [torch.cuda.Event() for _ in range(depth)]       # the successor's kernels have read it
                self.t_reader = [None] * depth          # the frame whose kernels read the slot's history
                self.t_tenant = [None] * depth          # the frame whose history the slot holds
                self.t_flow_live = [False] * depth      # the slot's frame came with a flow
                self.t_live = [False] * depth           # the slot's frame has values on their way home
                self.t_valid = [None] * depth           # the slot's forward-backward mask (flow_mask), while the frame is live
                self.t_stale = set()                    # frames done again by _redo: their history is not what was written
                # stabilise: the history's third plane, the frame as written, and the event behind the launch that fills it
                if self.stab_params is not None:
                    self.t_written = torch.empty((depth, height, width, 3), dtype=torch.uint8, device=self.device)
                    self.t_blended = [torch.cuda.Event() for _ in range(depth)]
            self.aff_len = [0] * depth
            self.drifts, self._last_aff = {}, None
            self.window_used = {}                  # frame index -> (frames pooled for record 0, frames the window held)
            # one StrengthMap per ring slot and the matte rings: made by the first run that needs them
            self.strength_maps = self.h_matte = None
            self.strength_on = False            # this run's frames have a strength map of their own
            self.strength_live = [False] * depth
            # one StyleMap per ring slot, the plane rings and the flag words: made by the first run (style_planes)
            self.style_maps = None
            self.style_live = [False] * depth
            self.redo_count = 0                 # frames done again on the dense route (more valid labels than the packed cap)
            self.mask_slots = None              # rings for per-frame label maps: made by the first run(..., masks=...)
            self.done = [torch.cuda.Event() for _ in range(depth)]
            self.consumed = [torch.cuda.Event() for _ in range(depth)]      # compute(i) has read d_in[slot]
        # where _submit records consumed[k]: behind the slot's last read.  A device resize reads the source slot (and the
        # planes' slot) right behind the upload; the encoder reads d_in[k]; and a late reader reads it behind the decode.
        # The Lab step reads d_in[k] after the decoder pass: the slot's last read is there, not at the encoder.  (A frame
        # done again by _redo reads it later still; that happens while the frame is retired, and run() retires the
        # slot's tenant - done[k].synchronize() - before it submits the next one.)  The guided upscale is under the
        # same rule: its fit reads d_in[k] and its apply kernel the source slot d_src[k], both behind the decoder pass.
        # So is the affinity loss, which reads d_in[k] (and d_src[k]) against the decoded frame, and the temporal loss,
        # which copies d_in[k] into the slot's history behind the decode.  A device resize with a late reader records
        # twice: the source slot's event behind the upload, then again behind the decode, which is the one the next
        # tenant waits for.  The content loss reads d_in[k] behind the decode as well.
        late = self.preserve_luminance or self.upscalers is not None or self.affinity_on or self.temporal_on
        late = late or (self.style_meters is not None and self.content_loss)
        if self.resizers is not None and self.upscalers is None:
            self.consumed_at = ("upload", "decode") if late else ("upload",)
        else:
            self.consumed_at = ("decode",) if late else ("encoder",)
        # the decode route of every frame: (k, z_cs) -> the uint8 frame, or None when the deep planes are on their way home
        if self.out_deep:
            self._decode_frame = self._decode_deep
        elif self.upscalers is not None:
            self._decode_frame = self._decode_guided
        elif not self.preserve_luminance:
            self._decode_frame = self._decode_plain
        elif self.custom_decode:
            self._decode_frame = self._decode_hook_lum
        else:
            self._decode_frame = self._decode_lum

    def _logit_rings(self):
        """The logit ring of a temporal window: R = seg_window + depth buffers of one frame's logits, one event per buffer, and
        one buffer per frame ring slot for the mixed logits."""
        from .segformer import SEG_CLASSES, window_weights
        if self.segmenter is None:
            raise ValueError("seg_window belongs to a segmenter")
        window_weights(self.seg_window, self.seg_decay)                  # (raises for a window or a decay out of range)
        hw, ww = (self.H, self.W) if self.seg_work is None else tuple(self.seg_work.shape[1:3])
        self.logit_grid = self.segmenter.logit_grid(hw, ww)
        cells = self.logit_grid[0] * self.logit_grid[1]
        slots = logit_ring_slots(self.seg_window, self.depth)
        need = (slots + self.depth) * cells * SEG_CLASSES * 4
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free // 2:
            raise ValueError(f"seg_window {self.seg_window} at depth {self.depth} holds {slots + self.depth} logit tensors of "
                             f"{self.logit_grid[0]}x{self.logit_grid[1]}x{SEG_CLASSES} floats ({need >> 20} MiB), more than half of "
                             f"the {free >> 20} MiB free on the device: segment at a working resolution (--seg_size), or lower "
                             "the window or the depth")
        self.logit_ring = torch.empty((slots, cells, SEG_CLASSES), dtype=torch.float32, device=self.device)
        self.logit_mix = torch.empty((self.depth, cells, SEG_CLASSES), dtype=torch.float32, device=self.device)
        self.logit_window = WindowRing(self.seg_window, self.depth, torch.cuda.Event, what="logit")

    def _stat_rings(self):
        """The record ring of a statistics window: R = logit_ring_slots(stats_window, depth) record buffers (made by the first
        frame, which tells their shape) with one event each, and per frame ring slot a pooled buffer and the `used` words."""
        self.stat_window = WindowRing(self.stats_window, self.depth, torch.cuda.Event)
        slots = self.stat_window.slots
        self.stat_ring = self.stat_pooled = self.d_used = self.h_used = None
        self.stat_ages = [1] * self.depth
        self.plan_ring = None
        if self.stats_by_label:                    # the packed masked route: N = 32, a block of 32 slot records per frame
            from . import _lib
            from .cwct import cWCT
            rec = 1 + 32 + 32 * 32
            self.stat_ring = torch.empty((slots, cWCT.MAX_SLOTS, rec), dtype=torch.float64, device=self.device)
            self.plan_ring = torch.empty((slots, _lib.LABEL_PLAN_BYTES), dtype=torch.uint8, device=self.device)
            self.stat_pooled = torch.empty((self.depth, cWCT.MAX_SLOTS, rec), dtype=torch.float64, device=self.device)
            self.d_used = torch.zeros((self.depth, cWCT.MAX_SLOTS), dtype=torch.int32, device=self.device)
            self.h_used, self.h_used_np = _pinned((self.depth, cWCT.MAX_SLOTS), torch.int32)

    def _label_slot(self, i):
        """The record ring slot frame i is about to write (statistics window by label)."""
        return self.stat_ring[self.stat_window.claim(i, self.last_retired)]

    def _label_window(self, i, k, sc, record, table):
        """Frame i's record block sits in ring slot i % R (queued on the current stream sc); its plan table goes next to it, then
        the slot's event, the waits for the W - 1 older frames' slots and the pool by label into the frame ring slot's buffer.

        The table must be copied: the frame's own plan buffer belongs to its FRAME ring slot and is overwritten `depth` frames
        later (or by the frame's own redo, with the dense plan), while the window reads it for W - 1 frames.  The event is
        recorded after both the record and the copy are queued, so a pool that waited for it reads a finished pair.  The ring
        and its invariant: WindowRing.  A frame with more than 8 valid labels leaves its cap-8 record and plan here as they
        are: right for the labels they hold, and an age a later frame skips for any other label."""
        from .cwct import cWCT
        j = i % self.stat_window.slots
        if record.data_ptr() != self.stat_ring[j].data_ptr():
            raise RuntimeError(f"frame {i}: its record was not written to the ring slot offered (record_out)")
        self.plan_ring[j].copy_(table, non_blocking=True)
        self.stat_window.publish(i, sc)
        order = self.stat_window.gather(i, sc)
        self.stat_ages[k] = len(order)
        return cWCT.pool_stats([self.stat_ring[jj] for jj in order], decay=self.stats_decay, cut=self.stats_cut,
                               out=self.stat_pooled[k], used=self.d_used[k], plans=[self.plan_ring[jj] for jj in order])

    def _stats_window(self, i, k, sc, z_c):
        """Frame i's record into ring slot i % R on the current stream sc, then the waits for the W - 1 older frames' records
        (one event per slot, recorded by their streams); returns the content_stats of the frame's transform.  The ring and its
        invariant: WindowRing.  The first frame of the pipeline makes the record ring: its record tells the shape."""
        j = self.stat_window.claim(i, self.last_retired)
        if self.stat_ring is None:                # the first frame of the pipeline: its record tells the shape
            first = self.frame_stats(z_c, out=None)
            self.stat_ring = torch.empty((self.stat_window.slots,) + tuple(first.shape), dtype=torch.float64, device=self.device)
            self.stat_pooled = torch.empty((self.depth,) + tuple(first.shape), dtype=torch.float64, device=self.device)
            n_rec = 1 if first.dim() == 1 else int(first.shape[0])
            self.d_used = torch.zeros((self.depth, n_rec), dtype=torch.int32, device=self.device)
            self.h_used, self.h_used_np = _pinned((self.depth, n_rec), torch.int32)
            self.stat_ring[j].copy_(first)
        else:
            self.frame_stats(z_c, out=self.stat_ring[j])
        self.stat_window.publish(i, sc)
        order = self.stat_window.gather(i, sc)
        self.stat_ages[k] = len(order)
        return _WindowStats(self, [self.stat_ring[jj] for jj in order], k)

    def _seg_source(self, k):
        """The segmenter's uint8 source for the frame in ring slot k: d_in[k][0], or - with a working size - the slot's working
        frame, made from it by resize_u8 on the current stream."""
        if self.seg_work is None:
            return self.d_in[k][0]
        from .resize import resize_u8
        work = self.seg_work[k]
        resize_u8(self.d_in[k][0], (work.shape[1], work.shape[0]), out=work, tmp=self.seg_tmp[k])
        return work

    def _frame_logits(self, i, k, sc):
        """The logits of the frame in ring slot k (frame i) into logit slot i % R, on the current stream sc, and the slot's
        event behind them (WindowRing)."""
        j = self.logit_window.claim(i, self.last_retired)
        self.segmenter.logits_into(self._seg_source(k), self.logit_ring[j])
        self.logit_window.publish(i, sc)
        return j

    def _segment_window(self, i, k, sc):
        """Frame i's label map from the window's mean logits, into the mask ring slot: this frame's logits into their ring
        slot, then - once the W - 1 older frames' logits are there, which their streams signal by one event per slot - the mix
        into the ring slot's scratch tensor and the sampling + argmax step of a plain run.  The ring and its invariant:
        WindowRing."""
        from .segformer import window_weights
        slot = self.mask_slots[k]
        slot.mask, slot.colours = self.d_mask[k, :self.H * self.W].view(self.H, self.W), False
        self._frame_logits(i, k, sc)
        order = self.logit_window.gather(i, sc)
        self.segmenter.mix_logits([self.logit_ring[j] for j in order], window_weights(len(order), self.seg_decay),
                                  self.logit_mix[k])
        self.segmenter.labels_from_logits(self.logit_mix[k], self.logit_grid, (self.H, self.W), out=slot.mask)
        return slot

    def _frame_mask(self, i, k, sc, mask):
        """Frame i's MaskSlot, filled on the current stream sc: segmented - per frame, or through the logit window -, uploaded
        (`mask`), or None for a frame without a label map."""
        if self.segmenter is not None:
            return self._segment_mask(k) if self.logit_window is None else self._segment_window(i, k, sc)
        return self._upload_mask(i, k, mask) if mask is not None else None

    def _mask_rings(self):
        """Pinned and device rings for one map per frame in flight (3 bytes per pixel: colours or labels fit), and the flag words."""
        if self.mask_slots is None:
            with torch.cuda.device(self.device):
                self.h_mask, self.h_mask_np = _pinned((self.depth, self.H * self.W * 3), torch.uint8)
                self.d_mask = torch.empty((self.depth, self.H * self.W * 3), dtype=torch.uint8, device=self.device)
                self.d_mflags = torch.zeros((self.depth, 1), dtype=torch.int32, device=self.device)
                self.h_mflags, self.h_mflags_np = _pinned((self.depth, 1), torch.int32)
                self.mask_slots = [MaskSlot(k, self.d_mflags[k]) for k in range(self.depth)]
        return self.mask_slots

    def _strength_rings(self, mattes):
        """One StrengthMap per ring slot and, for mattes, a pinned and a device ring (plus the resized ring and the resize's pass
        buffer when they arrive at another size); for colour maps a ring of label maps.  Slot reuse needs no event of its own:
        run() retires a slot's tenant (done[k].synchronize()) before it submits the next one, so nothing still reads the slot's
        matte or map when they are overwritten, and _redo runs while its frame is still the tenant: it reads the same map."""
        from .cwct import cWCT
        H, W, (Hm, Wm) = self.H, self.W, self.matte_hw
        with torch.cuda.device(self.device):
            if self.strength_maps is None:
                shape = (1, 32, H, W) if self.net.sp_steps == 2 else (1, 128, H // 2, W // 2)
                self.strength_maps = [cWCT.empty_strength(shape, self.device) for _ in range(self.depth)]
                self.d_slabels = (torch.empty((self.depth, H, W), dtype=torch.uint8, device=self.device)
                                  if self.strength_table is not None else None)
            if mattes and self.h_matte is None:
                self.h_matte, self.h_matte_np = _pinned((self.depth, Hm, Wm), torch.uint8)
                self.d_matte = torch.empty((self.depth, Hm, Wm), dtype=torch.uint8, device=self.device)
                self.d_matte_rs = self.d_matte_tmp = None
                if (Hm, Wm) != (H, W):
                    self.d_matte_rs = torch.empty((self.depth, H, W), dtype=torch.uint8, device=self.device)
                    self.d_matte_tmp = torch.empty((self.depth, Hm * W), dtype=torch.uint8, device=self.device)

    def _style_rings(self):
        """style_planes: per ring slot a StyleMap, a pinned and a device buffer for the frame's planes (plus the resized planes
        and the resize's pass buffer when they arrive at another size) and a flag word with its pinned twin.  Slot reuse needs
        no event of its own, for the reason _strength_rings gives: run() retires a slot's tenant (done[k].synchronize()) before
        it submits the next one, so nothing still reads the slot's planes, map or flag word when they are overwritten.  The
        flag word's copy home is queued behind the frame's, so it is there when the frame retires."""
        from .cwct import cWCT
        if self.style_maps is not None:
            return
        H, W, (Hm, Wm), P = self.H, self.W, self.style_hw, self.style_planes
        with torch.cuda.device(self.device):
            shape = (1, 32, H, W) if self.net.sp_steps == 2 else (1, 128, H // 2, W // 2)
            self.h_splanes, self.h_splanes_np = _pinned((self.depth, P, Hm, Wm), torch.uint8)
            self.d_splanes = torch.empty((self.depth, P, Hm, Wm), dtype=torch.uint8, device=self.device)
            self.d_splanes_rs = self.d_splanes_tmp = None
            if (Hm, Wm) != (H, W):
                self.d_splanes_rs = torch.empty((self.depth, P, H, W), dtype=torch.uint8, device=self.device)
                self.d_splanes_tmp = torch.empty((self.depth, Hm * W), dtype=torch.uint8, device=self.device)
            self.d_sflags = torch.zeros((self.depth, 1), dtype=torch.int32, device=self.device)
            self.h_sflags, self.h_sflags_np = _pinned((self.depth, 1), torch.int32)
            self.style_maps = [cWCT.empty_style_map(shape, 2 if P == 1 else P, self.device) for _ in range(self.depth)]

    def _frame_style_map(self, i, k, planes):
        """Frame i's StyleMap into ring slot k, queued on the current stream: the planes' upload (and resize, plane by plane), a
        clear of the slot's flag word, one vst_style_frame launch."""
        from .cwct import cWCT
        want = (self.style_planes,) + self.style_hw
        m = planes.numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
        if m.dtype != np.uint8 or m.shape != want:
            raise ValueError(f"frame {i}: its style planes must be uint8 {list(want)}, got {m.dtype} {tuple(m.shape)}")
        np.copyto(self.h_splanes_np[k], m)
        self.d_splanes[k].copy_(self.h_splanes[k], non_blocking=True)
        d = self.d_splanes[k]
        if self.d_splanes_rs is not None:
            from .resize import resize_grey_u8
            for p in range(self.style_planes):
                resize_grey_u8(d[p], (self.W, self.H), out=self.d_splanes_rs[k, p], tmp=self.d_splanes_tmp[k])
            d = self.d_splanes_rs[k]
        self.d_sflags[k].zero_()
        cWCT.frame_style_map(self.style_maps[k].code_shape, d, out=self.style_maps[k], flags=self.d_sflags[k])

    def _frame_strength(self, i, k, matte, mslot):
        """Frame i's StrengthMap into ring slot k, queued on the current stream: the matte's upload (and resize), the labels of
        the frame's MaskSlot as they are before any remapping, one vst_strength_frame launch."""
        from .cwct import cWCT
        d_matte, labels = self.static_matte, None
        if matte is not None:
            m = matte.numpy() if isinstance(matte, torch.Tensor) else np.asarray(matte)
            if m.dtype != np.uint8 or m.shape != self.matte_hw:
                raise ValueError(f"frame {i}: its matte must be uint8 [{self.matte_hw[0]},{self.matte_hw[1]}], got {m.dtype} "
                                 f"{tuple(m.shape)}")
            np.copyto(self.h_matte_np[k], m)
            self.d_matte[k].copy_(self.h_matte[k], non_blocking=True)
            d_matte = self.d_matte[k]
            if self.d_matte_rs is not None:
                from .resize import resize_grey_u8
                d_matte = resize_grey_u8(self.d_matte[k], (self.W, self.H), out=self.d_matte_rs[k], tmp=self.d_matte_tmp[k])
        if self.strength_table is not None:
            labels = mslot.mask if mslot is not None else self.static_labels
            if mslot is not None and mslot.colours:               # an uploaded colour map: through the dictionary, into the slot's own label map
                from . import _lib
                import ctypes as C
                labels = self.d_slabels[k]
                _lib.check(_lib.lib().vst_colors_to_labels(C.c_void_p(mslot.mask.data_ptr()), C.c_void_p(labels.data_ptr()),
                                                           self.H * self.W, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                           "vst_colors_to_labels")
        cWCT.frame_strength(self.strength_maps[k].code_shape, matte=d_matte, labels=labels, table=self.strength_table,
                            out=self.strength_maps[k])

    def _upload_mask(self, i, k, mask):
        """The frame's map into its pinned slot and (queued on the current stream) into its device slot."""
        m = mask.numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        if m.dtype != np.uint8 or m.shape[:2] != (self.H, self.W) or not (m.ndim == 2 or (m.ndim == 3 and m.shape[2] == 3)):
            raise ValueError(f"frame {i}: its label map must be uint8 [{self.H},{self.W}] or [{self.H},{self.W},3], got {m.dtype} "
                             f"{tuple(m.shape)}")
        slot = self.mask_slots[k]
        n = m.size
        np.copyto(self.h_mask_np[k, :n].reshape(m.shape), m)
        self.d_mask[k, :n].copy_(self.h_mask[k, :n], non_blocking=True)
        slot.mask, slot.colours = self.d_mask[k, :n].view(m.shape), m.ndim == 3
        return slot

    def _segment_mask(self, k):
        """The frame in ring slot k, segmented on the current stream into the slot's label map."""
        slot = self.mask_slots[k]
        slot.mask, slot.colours = self.d_mask[k, :self.H * self.W].view(self.H, self.W), False
        src = self._seg_source(k)
        if self.seg_work is None:
            self.segmenter.segment_u8(src, out=slot.mask)
        else:
            self.segmenter.segment_work_u8(src, (self.H, self.W), out=slot.mask)
        return slot

    def _upload(self, k):
        """The frame staged in pinned slot k up to the card and into the encoder's input d_in[k], queued on the current stream:
        the H2D copy - of the planes, with yuv_to_rgb_u8 behind it, under src_yuv - and the device resize if there is one."""
        rgb = self.d_in[k][0] if self.resizers is None else self.d_src[k]
        if self.src_deep:                   # the float planes for the encoder, and the same pixels as bytes for everything else
            from .yuv import yuv16_to_rgb_f32
            self.d_yuv[k].copy_(self.h_in[k], non_blocking=True)
            if self.deep_resizers is not None:      # source-size planes: the slot's resize makes both frames at the stylised size
                self.deep_resizers[k](self.d_yuv[k], out=self.d_xf[k], out_u8=rgb)
            else:
                yuv16_to_rgb_f32(self.d_yuv[k], self.H, self.W, self.src_yuv, out=self.d_xf[k], out_u8=rgb)
        elif self.src_yuv is not None:
            from .yuv import yuv_to_rgb_u8
            self.d_yuv[k].copy_(self.h_in[k], non_blocking=True)
            yuv_to_rgb_u8(self.d_yuv[k], self.Hs, self.Ws, self.src_yuv, out=rgb)
        else:
            rgb.copy_(self.h_in[k], non_blocking=True)
        if self.resizers is not None:       # the source-size frame went up, the encoder's input is made on the card
            self.resizers[k](self.d_src[k], self.d_in[k])

    def _encode(self, k):
        """The encoder pass of the frame in ring slot k, on the current stream: from the uint8 slot, or - a deep source - from
        the slot's float planes.  Every place that encodes a slot comes here."""
        return self.net(self.d_xf[k]) if self.src_deep else self.net.forward_u8(self.d_in[k])

    def _decode_deep(self, k, z_cs):
        """A deep out_yuv: the code to float planes, the Lab step, the resize to the written size, the conversion into the
        slot's flat buffer and that buffer's copy home, queued on the current stream; there is no uint8 frame to return."""
        from .yuv import rgb_f32_to_yuv16
        sty = self.net._inverse(z_cs, out=self.d_of[k])
        if self.preserve_luminance:
            from .color import luminance_transfer, luminance_transfer_u8
            if self.src_deep:
                sty = luminance_transfer(self.d_xf[k], sty, out=self.d_of_lum[k])
            else:
                luminance_transfer_u8(self.d_in[k], sty, out=sty, to_float=True)
        if self.d_of_rs is not None:
            from .resize import resize_f32
            sty = resize_f32(sty, (self.Ho, self.Wo), out=self.d_of_rs[k], tmp=self.d_of_tmp[k])
        self.h_out[k].copy_(rgb_f32_to_yuv16(sty, self.out_yuv, out=self.d_out_yuv[k]), non_blocking=True)

    def _decode_plain(self, k, z_cs):
        """The decoder pass, or the decode hook, straight to the uint8 frame."""
        return self.decode(z_cs)

    def _decode_hook_lum(self, k, z_cs):
        """preserve_luminance under a decode hook: the hook gets the frame's content slot."""
        return self.decode(z_cs, self.d_in[k])

    def _decode_lum(self, k, z_cs):
        """preserve_luminance: the decoder pass with the Lab step behind it, through the slot's float staging."""
        return self.net.inverse_u8(z_cs, luminance_of=self.d_in[k], scratch=self.lum_scratch[k])

    def _decode_guided(self, k, z_cs):
        """upscale='guided': the code to float planes at the working size, the Lab step, then the slot's GuidedUpscale - fit on
        (d_in[k], those planes), apply to d_src[k] - into the slot's source-size frame, queued on the current stream."""
        sty = self.net._inverse(z_cs, out=self.d_up[k])
        if self.preserve_luminance:
            from .color import luminance_transfer_u8
            luminance_transfer_u8(self.d_in[k], sty, out=sty, to_float=True)
        if self.affinity_on:                    # the float frame against the working-size content, before the writer's epilogue
            self.aff_work[k](self.d_in[k], sty, out=self.d_affinity[k, 0:3])
        out = self.upscalers[k](self.d_in[k], sty, self.d_src[k], out=self.d_up_out[k])
        if self.affinity_on:                    # the written full-size frame against the source frame
            self.aff_full[k](self.d_src[k], out, out=self.d_affinity[k, 3:6])
        return out

    def _stage(self, i, k, frame):
        """Frame i into the pinned slot k."""
        src = frame.numpy() if isinstance(frame, torch.Tensor) else np.asarray(frame)
        if src.shape != self.in_shape or src.dtype != np.uint8:
            what = f"[{self.Hs},{self.Ws},3]"
            if self.src_yuv is not None:
                what = f"[{self.in_shape[0]}] (the flat planes of a {self.Ws}x{self.Hs} frame)"
            raise ValueError(f"frame {i}: expected uint8 {what}, got {src.dtype} {tuple(src.shape)}")
        # plain single-threaded memcpy into the pinned slot.  (Not torch's CPU copy_: its intra-op thread pool spins after
        # every call and, inside a CPU-quota cgroup, throttles the thread that feeds the GPU — measured 9 ms vs 0.3 ms.)
        np.copyto(self.h_in_np[k], src)

    def _warm_slot(self, k):
        """A warm-up frame is not retired: the host waits for the one that last held ring slot k before the slot is filled again."""
        if k in self.warm_slots:
            self.done[k].synchronize()
            self.warm_slots.discard(k)

    def _warm(self, i, frame, upto, mask=None):
        """A warm-up frame of a window (frame i precedes the run's first frame): uploaded, resized if need be, and taken as far
        as `upto` says; it is not decoded and reaches no sink.
        "logits" (a temporal window): segmented as far as its logits, which go to their ring slot; it is not stylised.
        "record" (a statistics window): encoded and reduced into its ring slot.
        "label_record" (a statistics window by label): with its map - `mask`, or segmented, through the logit window if there
        is one -, encoded, planned and reduced into its ring slots by the transform itself - the plan is made there; the factor
        launch that follows is small.  Nor is it retired: its mask flag word is never read, so a warm-up map with more than 8
        valid labels just leaves its cap-8 record (as a frame of the run does), and one with a label outside the relation table
        (VST_MASK_OUT_OF_TABLE) passes silently here - the run that has that frame among its own frames is the one that raises
        for it."""
        k = i % self.depth
        self._warm_slot(k)
        sc = self.s_comp[i % len(self.s_comp)]
        self._stage(i, k, frame)
        with torch.cuda.device(self.device), torch.no_grad(), torch.cuda.stream(sc):
            self._upload(k)
            if upto == "logits":
                self._frame_logits(i, k, sc)
            elif upto == "record":
                self._stats_window(i, k, sc, self._encode(k))
            else:
                mslot = self._frame_mask(i, k, sc, mask)
                self.transform(self._encode(k), i, mslot, content_stats=_LabelWindowStats(self, i, k, sc))
            self.done[k].record(sc)
        self.warm_slots.add(k)

    def _submit(self, i, frame, mask=None, matte=None, flow=None, planes=None):
        k = i % self.depth
        self._warm_slot(k)
        self._stage(i, k, frame)
        sc = self.s_comp[i % len(self.s_comp)]
        with torch.cuda.device(self.device), torch.no_grad(), torch.cuda.stream(sc):
            if self.temporal_on:
                self._upload_flow(i, k, flow)
            # H2D, compute and D2H of one frame are queued on ONE stream (a uint8 frame is ~0.1 ms of PCIe time against
            # milliseconds of compute); overlap comes from consecutive frames being on different streams
            if i >= self.depth:
                sc.wait_event(self.consumed[k])                   # slot reuse: the previous tenant's encoder pass has read it
            self._upload(k)
            if "upload" in self.consumed_at:
                self.consumed[k].record(sc)                       # the source slot (and the planes' slot) has been read
            mslot = self._frame_mask(i, k, sc, mask)              # (on the frame's own stream)
            self.strength_live[k] = self.strength_on
            if self.strength_live[k]:
                self._frame_strength(i, k, matte, mslot)
            self.style_live[k] = planes is not None
            if self.style_live[k]:
                self._frame_style_map(i, k, planes)
            z_c = self._encode(k)
            if "encoder" in self.consumed_at:
                self.consumed[k].record(sc)
            window = None
            if self.stats_by_label:                 # (the plan is made inside the transform: so is everything else)
                window = _LabelWindowStats(self, i, k, sc)
            elif self.stats_window > 1:             # (never with a MaskSlot: the constructor and run() refuse those)
                window = self._stats_window(i, k, sc, z_c)
            self._finish(i, k, sc, z_c, self.transform, mslot, window)
            if "decode" in self.consumed_at:                      # a late reader: see the constructor
                self.consumed[k].record(sc)
            self.done[k].record(sc)

    def _finish(self, i, k, sc, z_c, transform, mslot, window=None, history=True):
        """cWCT, decoder pass, D2H copy and flag words of frame i, queued on the current stream (sc).  history=False (a frame
        done again): the temporal history keeps the first decode and nothing is measured."""
        # (a frame with a strength map of its own: one more keyword; otherwise the calls are exactly the plain ones)
        kw = dict(strength=self.strength_maps[k]) if self.strength_live[k] else {}
        if self.style_map is not None:
            if mslot is not None:
                raise ValueError("style maps are not supported on the masked routes")
            kw["style_map"] = self.style_map
        elif self.style_live[k]:                # (never with a MaskSlot: the constructor and run() refuse those)
            kw["style_map"] = self.style_maps[k]
        if window is not None:
            kw["content_stats"] = window
        z_cs = transform(z_c, i, **kw) if mslot is None else transform(z_c, i, mslot, **kw)
        if window is not None:
            self.h_used[k].copy_(self.d_used[k], non_blocking=True)
        if self.map_drift:
            self._affines_home(i, k, z_cs)
        out = self._decode_frame(k, z_cs)
        if self.stab_params is not None:        # (never with history=False: the constructor and run() refuse what _redo serves)
            self._history(i, k, sc, out)
            out = self._stabilise(i, k, sc)     # what every later step reads: the written bytes are the stabilised ones
        if self.affinity_on:
            if self.aff_full is None and out is not None and tuple(out.shape) == (1, self.Ho, self.Wo, 3) and out.dtype == torch.uint8:
                # a route that decodes straight to uint8: the decoded frame (before any YUV conversion) against the content
                self.aff_work[k](self.d_in[k], out.contiguous(), out=self.d_affinity[k, 0:3])
            self.h_affinity[k].copy_(self.d_affinity[k], non_blocking=True)
        if self.style_meters is not None:       # the frame the sink receives (a frame done again: its second decode)
            if out is None or tuple(out.shape) != (1, self.Ho, self.Wo, 3) or out.dtype != torch.uint8:
                raise RuntimeError(f"frame {i}: the style loss needs a decoded uint8 (1,{self.Ho},{self.Wo},3) frame")
            self.style_meters[k](out.contiguous(), self.d_in[k] if self.content_loss else None, out=self.d_style[k])
            self.h_style[k].copy_(self.d_style[k], non_blocking=True)
        if self.temporal_on and history:
            if self.stab_params is None:
                self._history(i, k, sc, out)
            self._temporal(i, k, sc)
        if out is None:                     # (the deep planes are on their way home)
            pass
        elif tuple(out.shape) != (1, self.Ho, self.Wo, 3) or out.dtype != torch.uint8:
            raise RuntimeError(f"decode returned {out.dtype} {tuple(out.shape)}, expected uint8 (1,{self.Ho},{self.Wo},3)")
        elif self.out_yuv is not None:        # the planes are what goes home
            from .yuv import rgb_to_yuv_u8
            self.h_out[k].copy_(rgb_to_yuv_u8(out.contiguous(), self.out_yuv, out=self.d_out_yuv[k]), non_blocking=True)
        else:
            self.h_out[k].copy_(out[0], non_blocking=True)
        if self.style_live[k]:
            self.h_sflags[k].copy_(self.d_sflags[k], non_blocking=True)
        self.flag_check[k] = getattr(self.net, "resolved_precision", None) in ("f16x2", "f16x2h")
        if self.flag_check[k]:
            from . import _lib
            import ctypes as C
            _lib.check(_lib.lib().vst_range_flags_async(C.c_void_p(self.d_flags[k].data_ptr()), C.c_void_p(sc.cuda_stream)),
                       "vst_range_flags_async")
            self.h_flags[k].copy_(self.d_flags[k], non_blocking=True)
        self.mask_check[k] = mslot is not None
        if mslot is not None:
            self.h_mflags[k].copy_(self.d_mflags[k], non_blocking=True)
            if self.mask_sink is not None:
                m = mslot.mask if self.mask_map is None else self.mask_map(mslot)
                if m.dtype != torch.uint8 or tuple(m.shape) != (self.H, self.W):
                    raise RuntimeError(f"the map for mask_sink must be uint8 [{self.H},{self.W}], got {m.dtype} {tuple(m.shape)}")
                self.h_seg[k].copy_(m, non_blocking=True)

    def _upload_flow(self, i, k, flow):
        """Frame i's flow into ring slot k's device buffer, queued on the current stream (a host array through the pinned
        slot).  The buffer's last reader was frame i - depth, which run() retired before it submitted this frame."""
        self.t_flow_live[k] = flow is not None or self.flow_estimate    # (estimated: _temporal fills the slot's buffer)
        if flow is None or self.flow_estimate:
            return
        want = (2, self.H, self.W)
        if torch.is_tensor(flow) and flow.is_cuda:
            if flow.dtype != torch.float32 or tuple(flow.shape) != want or flow.device != self.t_flow.device:
                raise ValueError(f"frame {i}: its flow must be float32 {list(want)} on {self.device}, got {flow.dtype} "
                                 f"{tuple(flow.shape)} on {flow.device}")
            self.t_flow[k].copy_(flow, non_blocking=True)
            return
        f = flow.numpy() if torch.is_tensor(flow) else np.asarray(flow)
        if f.dtype != np.float32 or f.shape != want:
            raise ValueError(f"frame {i}: its flow must be float32 {list(want)}, got {f.dtype} {tuple(f.shape)}")
        np.copyto(self.t_flow_h_np[k], f)
        self.t_flow[k].copy_(self.t_flow_h[k], non_blocking=True)

    def _history(self, i, k, sc, out):
        """The first half of _temporal (see there): frame i's history into ring slot k, the slot's "written" event, whether the
        frame has values to come, the wait for frame i - 1's history and, with flow="estimate", the frame's flow (and mask)."""
        if out is None or tuple(out.shape) != (1, self.H, self.W, 3) or out.dtype != torch.uint8:
            raise RuntimeError(f"frame {i}: the temporal loss needs a decoded uint8 (1,{self.H},{self.W},3) frame")
        reader = self.t_reader[k]
        if reader is not None:                      # (the successor of the slot's previous tenant)
            assert reader < i, f"history slot {k}: frame {reader} reads what frame {i} is about to overwrite"
            sc.wait_event(self.t_read[k])
            self.t_reader[k] = None
        self.t_in[k].copy_(self.d_in[k][0], non_blocking=True)
        self.t_out[k].copy_(out[0], non_blocking=True)
        self.t_ready[k].record(sc)
        self.t_tenant[k] = i
        kp = (i - 1) % self.depth
        self.t_live[k] = self.t_flow_live[k] and self.t_tenant[kp] == i - 1
        self.t_valid[k] = None
        if self.t_live[k]:
            sc.wait_event(self.t_ready[kp])
            if self.flow_estimate:                  # on the input pair, behind the wait: ref = frame i, src = frame i - 1
                if self.flow_mask:
                    self.t_valid[k] = self.t_estimators[k].masked(self.t_in[k], self.t_in[kp], out=self.t_flow[k])[1]
                else:
                    self.t_estimators[k](self.t_in[k], self.t_in[kp], out=self.t_flow[k])

    def _stabilise(self, i, k, sc):
        """Frame i as it is written, into t_written[k], queued on sc behind _history: the blend of t_out[k] with frame i - 1's
        t_written under this frame's flow (see _temporal for the ordering), or a copy of t_out[k] for a frame that is not live.
        Returns the plane as the (1,H,W,3) frame the later steps read."""
        kp = (i - 1) % self.depth
        if self.t_live[k]:
            from .stabilise import stabilise
            sc.wait_event(self.t_blended[kp])
            stabilise(self.t_in[k], self.t_in[kp], self.t_out[k], self.t_written[kp], self.t_flow[k], valid=self.t_valid[k],
                      out=self.t_written[k], **self.stab_params)
        else:
            self.t_written[k].copy_(self.t_out[k], non_blocking=True)
        self.t_blended[k].record(sc)
        return self.t_written[k].unsqueeze(0)

    def _temporal(self, i, k, sc):
        """Frame i's history into ring slot k - a copy of the encoder's input d_in[k] and of the decoded uint8 frame `out`,
        queued on the current stream sc behind the decode - then the slot's "written" event, the wait for frame i - 1's, the
        two L1 launches against slot (i - 1) % depth under this frame's flow, and that slot's "read" event.

        The ring invariant is that of WindowRing with a window of two: slot k was written by frame i - depth and read by
        frame i - depth + 1 alone.  run() retires frame i - depth before it submits frame i, which completes that frame's own
        work, but not its successor's: frame i - depth + 1 may still be in flight (depth >= 2 puts it at or before frame i - 1,
        so it has been submitted and its "read" event recorded).  So this frame waits for t_read[k] before the copies: the
        one ordering the retire rule does not give.  Everything else the frame touches here - the flow buffer, the meter's
        workspace, the six values - belongs to the slot and was last used by frame i - depth itself.

        flow="estimate": behind the wait for t_ready[kp] the slot's FlowEstimator fills t_flow[k] from (t_in[k], t_in[kp]) - and,
        with flow_mask, the slot's backward flow and mask - before the two L1 launches; estimator, backward flow and mask belong
        to the slot like the meter's workspace, and t_read[kp] is still recorded behind the last launch that reads slot kp.

        The work is queued in two halves: _history (the copies, the two events' waits, the estimator) and this method (the L1
        launches, t_read[kp], the copy home).  Without stabilise one follows the other here, behind the affinity loss.

        stabilise: _history and _stabilise run right behind the decode instead, and the slot has a third plane, t_written[k].
        Its invariant: t_written[k] is written by frame i's blend (or copy) alone, after that frame has waited for t_read[k] -
        so frame i - depth + 1, the one reader of the slot's previous tenant, has finished with all three planes - and it is
        read by frame i's later steps on sc and by frame i + 1's blend and L1 launches, which record t_read[k] behind them as
        for the other two planes.  The recursion's own ordering - frame i's blend reads t_written[kp], so it must follow frame
        i - 1's blend - has an event of its own, t_blended[k], recorded behind the blend and waited for by frame i + 1 just
        before its blend.  t_ready[k] stays where it was, behind the two copies: recording it behind the blend instead would
        make frame i + 1's flow estimator, which needs nothing but t_in[k], wait for the whole chain of blends before it, and
        the estimators of consecutive frames - the longest step the flag adds to a frame's stream - would no longer overlap.
        The blends themselves form a chain by nature; each is one short launch.  loss_out is then measured on the written
        pair (t_written) and a third call measures the decoder's pair (t_out) into the slot's third row of values."""
        kp = (i - 1) % self.depth
        if self.t_live[k]:
            valid = self.t_valid[k]
            if self.stab_params is not None:        # (behind the wait for t_blended[kp]: _stabilise, on this stream)
                self.t_meters[k](self.t_written[kp], self.t_written[k], self.t_flow[k], out=self.d_temporal[k, 0], valid=valid)
                self.t_meters[k](self.t_out[kp], self.t_out[k], self.t_flow[k], out=self.d_temporal[k, 2], valid=valid)
            else:
                self.t_meters[k](self.t_out[kp], self.t_out[k], self.t_flow[k], out=self.d_temporal[k, 0], valid=valid)
            self.t_meters[k](self.t_in[kp], self.t_in[k], self.t_flow[k], out=self.d_temporal[k, 1], valid=valid)
            self.t_read[kp].record(sc)
            self.t_reader[kp] = i
            self.h_temporal[k].copy_(self.d_temporal[k], non_blocking=True)

    def _affines_home(self, i, k, z_cs):
        """map_drift: the frame's pending affine record(s) into the pinned ring, queued on the current stream."""
        from .code import PackedCode
        aff = None
        if isinstance(z_cs, PackedCode) and z_cs.pending_affines is not None:
            aff = z_cs.pending_affines.reshape(-1)
        elif isinstance(z_cs, PackedCode) and z_cs.pending_labels is not None:
            per_image, ms = z_cs.pending_labels
            if not 1 <= int(ms) <= 32:
                raise RuntimeError("map_drift on a masked route needs the plan's slot count (cWCT.learn_slots)")
            a = per_image[0][0].reshape(-1)
            aff = a[:int(ms) * (a.numel() // 32)]
        if aff is None:
            raise RuntimeError(f"frame {i}: map_drift needs a transform that returns a PackedCode with a pending map")
        if self.h_aff is None or self.h_aff.shape[1] < aff.numel():
            self.h_aff, self.h_aff_np = _pinned((self.depth, aff.numel()), torch.float32)
        self.aff_len[k] = aff.numel()
        self.h_aff[k, :aff.numel()].copy_(aff, non_blocking=True)

    def _redo(self, i, k):
        """Frame i had more valid labels than the packed route's slots: once more from the uploaded frame (its ring slots are
        still its own), with the `redo` transform (the dense route) and the same decode, before it goes to the sink.  Slow and
        correct."""
        if self.redo is None:
            raise RuntimeError(f"frame {i}: more valid labels than the masked route's slots and no redo transform was given")
        sc = self.s_comp[i % len(self.s_comp)]
        if self.temporal_on:                        # the history holds the first decode, not the one that is written
            self.t_stale.add(i)
        with torch.cuda.device(self.device), torch.no_grad(), torch.cuda.stream(sc):
            self._finish(i, k, sc, self._encode(k), self.redo, self.mask_slots[k], history=False)
            self.done[k].record(sc)
        self.done[k].synchronize()
        self.redo_count += 1

    def _retire(self, i, sink):
        k = i % self.depth
        self.done[k].synchronize()
        self.last_retired = i
        if self.mask_check[k] and self.h_mflags_np[k, 0]:
            from . import _lib
            flags = int(self.h_mflags_np[k, 0])
            if flags & _lib.MASK_OUT_OF_TABLE:
                raise RuntimeError(f"frame {i}: a label of its map needs the relation table but lies outside it")
            if flags & _lib.MASK_OVERFLOW:
                self._redo(i, k)
                if self.h_mflags_np[k, 0] & _lib.MASK_OVERFLOW:
                    raise RuntimeError(f"frame {i}: more than 32 valid labels")
        if self.style_live[k] and self.h_sflags_np[k, 0] & 1:
            raise StyleMapZeroSum(i)
        if self.flag_check[k] and self.h_flags_np[k].any():
            flags = int(np.bitwise_or.reduce(self.h_flags_np[k]))
            raise RuntimeError(f"frame {i}: fp16 range flags 0x{flags:x} raised by precision='{self.net.resolved_precision}' "
                               "(1 = an activation saturated at +-65504): this checkpoint / input needs precision='bf16x3'")
        if self.stats_by_label:                     # the least any live label pooled (0: no label had a usable record)
            live = self.h_used_np[k][self.h_used_np[k] > 0]
            self.window_used[i] = (int(live.min()) if live.size else 0, self.stat_ages[k])
            self.pooled_frames += int(live.sum())
            self.pooled_labels += int(live.size)
        elif self.stats_window > 1:
            self.window_used[i] = (int(self.h_used_np[k, 0]), self.stat_ages[k])
        if self.map_drift:
            a = self.h_aff_np[k, :self.aff_len[k]].astype(np.float64)
            if self._last_aff is not None and self._last_aff.shape == a.shape:
                self.drifts[i] = float(np.linalg.norm(a - self._last_aff) / np.linalg.norm(a))
            self._last_aff = a
        if self.affinity_on:
            self.affinity[i] = self.h_affinity_np[k].copy()
        if self.style_meters is not None:
            self.style[i] = tuple(float(v) for v in self.h_style_np[k])
        if self.temporal_on and self.t_live[k]:
            from .temporal import mean3
            stale = i in self.t_stale or (i - 1) in self.t_stale
            row = (float("nan") if stale else mean3(self.h_temporal_np[k, 0, :3]), mean3(self.h_temporal_np[k, 1, :3]))
            self.temporal[i] = row + (float(self.h_temporal_np[k, 1, 3]),) if self.flow_mask else row
            if self.stab_params is not None:
                self.stabilised[i] = mean3(self.h_temporal_np[k, 2, :3])
        if self.mask_check[k] and self.mask_sink is not None:
            self.mask_sink(i, self.h_seg_np[k])
        sink(i, self.h_out_np[k])        # a view of the pinned slot: valid until `depth` more frames are submitted

    @property
    def mean_drift(self):
        """map_drift: the mean of the last run's per-frame drifts (0.0 before two frames have retired)"""
        return float(np.mean(list(self.drifts.values()))) if self.drifts else 0.0

    @property
    def stats_cuts(self):
        """frames of the last run whose window was cut at age 1: record 0 (stats_by_label: no live label) pooled nothing while
        older frames existed"""
        return sum(1 for used, ages in self.window_used.values() if used == 1 and ages > 1)

    def run(self, frames, sink, start_index=0, masks=None, warmup=(), mattes=None, warmup_masks=None, flows=None,
            style_maps=None):
        """frames: iterable of uint8 HWC arrays/tensors (src_yuv: flat planes); sink(index, uint8 HWC numpy view - out_yuv: the flat
        planes) is called in frame order
        from this thread (copy or encode before returning).  Returns the number of frames processed.
        masks: optional iterable, one label map per frame (uint8 [H,W] labels or [H,W,3] colours at the frame's size), taken
        in step with `frames`; transform is then called with the frame's MaskSlot as third argument.
        warmup: with seg_window = W > 1, the up to W - 1 frames that precede frame `start_index` in the clip, oldest first.  They
        are segmented as far as their logits only, so that the first frames of this run (a shard of a clip) see the window a
        single run over the whole clip gives them.  A run without them starts its window at its own first frame.  With
        stats_window = W > 1 they are encoded and reduced to their records instead (one encoder pass each), to the same end.
        stats_by_label: warmup may hold (seg_window - 1) + (stats_window - 1) frames.  The newest stats_window - 1 of them are
        segmented (through the logit window) or uploaded with their maps - warmup_masks, one per warm-up frame, with `masks` -,
        encoded, planned and reduced into the record ring; the older ones go as far as their logits (warmup_counts).
        mattes: optional iterable, one uint8 [Hm,Wm] grey matte per frame (matte_hw; default the frame's size), taken in step with
        `frames`: the frame's strength map is v / 255, times table[label] with a strength_table.
        flows (temporal=True): an iterable in step with `frames`; an entry is the frame's flow, float32 [2,H,W] as a host array
        or a tensor on this device - the frame before it sampled at x - flow(x) predicts this frame -, or None for a frame
        without a predecessor or without a value.  The first frame of a run has no value whatever its entry says.
        style_maps (style_planes=P): an iterable, one uint8 [P,Hm,Wm] array of grey planes per frame (style_hw; default the
        frame's size), taken in step with `frames`; transform is then called with style_map=<the frame's StyleMap>."""
        if (style_maps is not None) != (self.style_planes is not None):
            raise ValueError("run(..., style_maps=...) goes with a pipeline made with style_planes, and such a pipeline needs it")
        if style_maps is not None and masks is not None:
            raise ValueError("style maps are not supported on the masked routes")
        if masks is not None and self.stab_params is not None:
            raise ValueError("stabilise does not go with per-frame mask slots (run(..., masks=...) or a segmenter): a frame done "
                             "again when it retires would leave a stale frame in the recursion")
        if (flows is not None) != (self.temporal_on and not self.flow_estimate):
            raise ValueError("run(..., flows=...) goes with a pipeline made with temporal=True, and such a pipeline needs it "
                             "unless it estimates its flows (flow='estimate'), which takes none")
        n = 0
        warmup = list(warmup)
        most = (self.seg_window - 1) + (self.stats_window - 1)      # (without stats_by_label one of the two is 0)
        if len(warmup) > most:
            what = "(seg_window - 1) + (stats_window - 1)" if self.stats_by_label else "seg_window - 1"
            raise ValueError(f"warmup holds at most {what} = {most} frames, got {len(warmup)}")
        if masks is not None and self.stats_window > 1 and not self.stats_by_label:
            raise ValueError("stats_window does not go with per-frame label maps: the label slots differ from frame to frame")
        if self.stats_by_label:
            if masks is None and self.segmenter is None:
                raise ValueError("stats_by_label needs per-frame label maps: `masks` or a segmenter")
            warmup_masks = list(warmup_masks) if warmup_masks is not None else []
            if masks is not None and len(warmup_masks) != len(warmup):
                raise ValueError(f"warmup_masks: one label map per warm-up frame, got {len(warmup_masks)} for {len(warmup)}")
        elif warmup_masks is not None:
            raise ValueError("warmup_masks belongs to stats_by_label")
        lag = self.depth - 1
        masks_it = None
        if masks is not None and self.segmenter is not None:
            raise ValueError("label maps come from the segmenter or from `masks`, not both")
        if masks is not None:
            masks_it = iter(masks)
        if masks is not None or self.segmenter is not None:
            self._mask_rings()
        elif self.strength_table is not None and self.static_labels is None:
            raise ValueError("strength_table needs a label source: `masks`, a segmenter or static_labels")
        mattes_it = iter(mattes) if mattes is not None else None
        flows_it = iter(flows) if flows is not None else None
        planes_it = iter(style_maps) if style_maps is not None else None
        if planes_it is not None:
            self._style_rings()
        if self.temporal_on:                        # a run is one history: nothing of an earlier run is anybody's predecessor
            self.temporal, self.stabilised, self.t_stale = {}, {}, set()
            self.t_tenant, self.t_reader = [None] * self.depth, [None] * self.depth
            self.t_live = [False] * self.depth
        self.strength_on = mattes is not None or self.strength_table is not None
        if self.strength_on:
            self._strength_rings(mattes is not None)
        with torch.cuda.device(self.device):       # whatever the caller queued so far (style code, statistics) comes first
            ev0 = torch.cuda.Event()
            ev0.record(torch.cuda.current_stream())
            for st in self.s_comp:
                st.wait_event(ev0)
        # the newest stats_window - 1 warm-up frames go as far as their records (without a statistics window: none), the older
        # ones - stats_by_label under a seg_window, or a seg_window alone - as far as their logits
        n_stat = min(len(warmup), self.stats_window - 1) if self.stat_window is not None else 0
        n_logit = len(warmup) - n_stat
        self.last_retired = None
        if self.logit_window is not None:           # a run is one window history: it starts at its oldest warm-up frame
            self.logit_window.start(start_index - len(warmup))
            for j, frame in enumerate(warmup[:n_logit]):
                self._warm(start_index - len(warmup) + j, frame, "logits")
        elif self.stats_by_label and n_logit:
            raise ValueError(f"warmup holds at most stats_window - 1 = {self.stats_window - 1} frames without a seg_window, got "
                             f"{len(warmup)}")
        self.drifts, self._last_aff, self.window_used = {}, None, {}
        self.affinity = {}
        self.style = {}
        self.pooled_frames = self.pooled_labels = 0     # stats_by_label: frames pooled, summed over the live labels of the run
        if self.stat_window is not None:            # a run is one window history, as above
            self.stat_window.start(start_index - n_stat)
            for j in range(n_stat):
                self._warm(start_index - n_stat + j, warmup[n_logit + j], "label_record" if self.stats_by_label else "record",
                           warmup_masks[n_logit + j] if masks is not None else None)
        for frame in frames:
            # slot (n % depth) was last used by frame n-depth, which was retired in the previous iteration
            i = start_index + n
            mask = _next_entry(masks_it, i, "label map (masks ran out)")
            matte = _next_entry(mattes_it, i, "matte (mattes ran out)")
            flow = _next_entry(flows_it, i, "flow entry (flows ran out)")
            planes = _next_entry(planes_it, i, "style planes (style_maps ran out)")
            self._submit(i, frame, mask, matte, flow, planes)
            n += 1
            if n > lag:
                self._retire(start_index + n - 1 - lag, sink)
        for j in range(max(0, n - lag), n):
            self._retire(start_index + j, sink)
        return n


def prefetch(source, ahead=4):
    """Iterate `source` in a background thread, up to `ahead` items ahead of the consumer; exceptions are re-raised
    in the consumer."""
    q: queue.Queue = queue.Queue(maxsize=max(1, ahead))
    end = object()
    stop = threading.Event()            # set when the consumer stops early (exception, break, generator close)

    def put(item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def work():
        try:
            for item in source:
                if not put(item):
                    return              # consumer is gone: drop the decoded frames, end the thread
            put(end)
        except BaseException as e:      # noqa: BLE001 — handed to the consumer
            put(e)

    t = threading.Thread(target=work, daemon=True)
    t.start()
    try:
        while True:
            item = q.get()
            if item is end:
                break
            if isinstance(item, BaseException):
                raise item
            yield item
    finally:
        stop.set()
        while True:                     # release whatever the producer had queued
            try:
                q.get_nowait()
            except queue.Empty:
                break
        t.join(timeout=5.0)


def parallel_map(fn, items, workers=4, ahead=8):
    """fn(item) for every item on `workers` threads, results yielded IN ORDER, at most `ahead` + `workers` items in flight
    (bounded memory: a decoded 1080p frame is 6 MB).  PIL's decoders, resizers and numpy copies release the GIL, so the frames
    of a clip decode on several cores while one thread feeds the GPU.  An exception of fn is re-raised at its item's turn."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    if workers <= 1:
        for item in items:
            yield fn(item)
        return
    pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="vst-decode")
    pending = deque()
    try:
        it = iter(items)
        for item in it:
            pending.append(pool.submit(fn, item))
            if len(pending) >= ahead + workers:
                yield pending.popleft().result()
        while pending:
            yield pending.popleft().result()
    finally:
        for f in pending:
            f.cancel()
        pool.shutdown(wait=True)


def host_cores():
    """cores this process may use: the usable cores (affinity mask, cgroup quota), capped by the per-rank thread cap that
    launch_children sets in OMP_NUM_THREADS"""
    import os
    from .sharding import usable_cores
    n = usable_cores()
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        n = min(n, int(os.environ["OMP_NUM_THREADS"]))
    return max(1, n)


def host_workers(requested=0):
    """(decode threads, encode threads) of the video loop: `requested` of each, or a split of this process's cores that leaves
    one for the thread that feeds the GPU - a frame's PNG encode costs several times its decode + resize"""
    if requested > 0:
        return requested, requested
    n = host_cores() - 1
    dec = max(1, min(4, n // 4))
    return dec, max(1, min(12, n - dec))


def save_png(path, frame, level=0):
    """uint8 [H,W,3] -> a PNG file.  level 0: this module's own writer - unfiltered rows in stored deflate blocks (a valid,
    lossless PNG of 3 bytes per pixel + 0.02 %): a few milliseconds per 1080p frame where PIL's encoder spends 50-140 ms on row
    filters even at compress_level 0; the zlib / crc32 calls release the GIL, so several sink threads scale.  level 1-9: PIL with
    that zlib level (filters + deflate: ~30 % smaller files on photographic content, 10-30x the time)."""
    import struct
    import zlib
    arr = np.ascontiguousarray(frame, dtype=np.uint8)
    if level > 0 or arr.ndim != 3 or arr.shape[2] != 3:
        from PIL import Image
        Image.fromarray(arr).save(path, format="PNG", compress_level=max(0, level))
        return
    h, w, _ = arr.shape
    raw = np.empty((h, 1 + 3 * w), np.uint8)
    raw[:, 0] = 0                                           # filter type 0 (none) in front of every row
    raw[:, 1:] = arr.reshape(h, 3 * w)
    data = zlib.compress(raw, 0)

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(tag)) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        f.write(struct.pack(">I", len(data)) + b"IDAT")
        f.write(data)
        f.write(struct.pack(">I", zlib.crc32(data, zlib.crc32(b"IDAT")) & 0xFFFFFFFF) + chunk(b"IEND", b""))


class AsyncSink:
    """Run a sink (frame encode / file write) on background threads; frames are copied out of the pinned slot first.
    workers = 1: one thread, frames reach `fn` in order (a video writer).  workers > 1: `fn` is called concurrently and in any
    order - for sinks whose calls are independent (one numbered PNG per frame: the encode of a 1080p frame is tens of
    milliseconds on one core, several times the GPU time of the frame).  close() waits for the queue to drain and re-raises the
    first writer error."""

    def __init__(self, fn, ahead=8, workers=1):
        self.fn = fn
        self.q: queue.Queue = queue.Queue(maxsize=max(1, ahead, 2 * workers))
        self.err = None
        self.threads = [threading.Thread(target=self._work, daemon=True, name=f"vst-sink-{k}") for k in range(max(1, workers))]
        for t in self.threads:
            t.start()

    def _work(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            if self.err is None:
                try:
                    self.fn(*item)
                except BaseException as e:      # noqa: BLE001
                    self.err = e

    def __call__(self, index, frame):
        if self.err is not None:
            raise self.err
        self.q.put((index, np.array(frame, copy=True)))

    def close(self):
        for _ in self.threads:
            self.q.put(None)
        for t in self.threads:
            t.join()
        if self.err is not None:
            raise self.err
