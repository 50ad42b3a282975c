"""Frames/s of the masked video path with ONE LABEL MAP PER FRAME, against the static-plan path.

    python tools/bench_masks.py [--frames 300] [--height 1080 --width 1920] [--labels 5] [--streams 3] [--host-frames 60]

Photorealistic, 5-label colour band maps that shift by a few pixels per frame, three streams.  Three ways to run the clip:
  (a) static   one map for every frame: plan_masks -> learn_slots -> bind_style once (what the pipeline did before)
  (b) device   a new map per frame through the device producers (cWCT.plan_frame, csrc/masks.hip), with remapping
  (c) host     a new map per frame through the host functions (colors_to_labels, SegReMapping, plan_masks, learn_slots,
               bind_style per frame): what a caller had to write without (b)
each as the host-pipeline rate (FramePipeline.run: pinned frames in, pinned frames out, wall clock) and, for (a) and (b), as
the device-resident rate (frames and maps already on the card, HIP events around the whole loop).  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from utils.utils import SEG_COLORS, colors_to_labels                    # noqa: E402
from vstnet_amd.synth import synthetic_state_dict, synthetic_frames     # noqa: E402


def band_map(h, w, k, shift):
    out = np.zeros((h, w, 3), np.uint8)
    edges = np.linspace(0, w, k + 1).astype(int)
    for i in range(k):
        out[:, edges[i]:edges[i + 1]] = SEG_COLORS[i][0]
    return np.ascontiguousarray(np.roll(out, shift, axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--host-frames", type=int, default=60, help="frames of the (slow) host variant (c)")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--labels", type=int, default=5)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--only", default="abc")
    args = ap.parse_args()
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from models.segmentation.SegReMapping import SegReMapping
    from vstnet_amd.masks import DeviceSegReMapping
    from vstnet_amd.pipeline import FramePipeline
    H, W, K = args.height, args.width, args.labels
    dev = torch.device("cuda")
    net = RevResNet(hidden_dim=16, sp_steps=2, precision=args.precision)
    net.load_state_dict(synthetic_state_dict(1234, 16, 2))
    net = net.to(dev).eval()
    cw = cWCT(precision=args.precision)
    table = np.load(os.path.join(REPO, "tests", "golden", "segremap.npz"))["mapping"]
    frames = [(synthetic_frames(1, H, W, seed=40 + i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(4)]
    maps = [band_map(H, W, K, 4 * i) for i in range(16)]                 # shifts by 4 pixels per frame, cycled
    style_rgb = band_map(H, W, K, 0)[:, ::-1].copy()
    host_remap = SegReMapping(table.astype(np.int64), 0.01)
    sseg = host_remap.self_remapping(colors_to_labels(style_rgb))
    with torch.no_grad():
        z_s = net.forward_u8((synthetic_frames(1, H, W, seed=9).permute(0, 2, 3, 1) * 255).byte().to(dev))
        static = cw.bind_style(cw.learn_slots(cw.plan_masks(colors_to_labels(maps[0])[None], sseg[None], (1, 32, H, W),
                                                            z_s.shape, dev)), z_s)
        binding = cw.bind_style_labels(z_s, sseg)
    remap = DeviceSegReMapping(table, 0.01)

    def t_static(z, i, ms=None):
        return cw.transfer_with_plan(z, None, static)

    def t_device(z, i, ms):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, dev)
        return cw.transfer_with_plan(z, None, cw.plan_frame(ms.mask, binding, remap=remap, colours=ms.colours, max_slots=8,
                                                            buffers=buf, flags=ms.flags))

    def t_host(z, i, ms=None):          # everything a per-frame map needs, with the host functions
        seg = colors_to_labels(maps[i % len(maps)])
        seg = host_remap.cross_remapping(host_remap.self_remapping(seg), sseg)
        plan = cw.bind_style(cw.learn_slots(cw.plan_masks(seg[None], sseg[None], (1, 32, H, W), z_s.shape, dev)), z_s)
        return cw.transfer_with_plan(z, None, plan)

    def pipeline_rate(transform, n, with_masks):
        pipe = FramePipeline(net, transform, H, W, device=dev, depth=6, compute_streams=args.streams)
        src = lambda m: (frames[i % len(frames)] for i in range(m))                    # noqa: E731
        msk = lambda m: (maps[i % len(maps)] for i in range(m)) if with_masks else None     # noqa: E731
        pipe.run(src(args.warmup), lambda i, f: None, masks=msk(args.warmup))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.run(src(n), lambda i, f: None, masks=msk(n))
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), pipe.redo_count

    def resident_rate(per_frame, n):
        """frames and maps on the card; frame i on stream i % streams; HIP events around the loop"""
        from vstnet_amd.pipeline import MaskSlot
        streams = [torch.cuda.Stream(device=dev) for _ in range(args.streams)]
        d_frames = [torch.from_numpy(f)[None].to(dev) for f in frames]
        d_maps = [torch.from_numpy(m).to(dev) for m in maps]
        ring = 2 * args.streams
        slots = [MaskSlot(k, torch.zeros(1, dtype=torch.int32, device=dev)) for k in range(ring)]
        outs = [None] * ring

        def loop(m):
            for i in range(m):
                st = streams[i % len(streams)]
                with torch.cuda.stream(st), torch.no_grad():
                    z = net.forward_u8(d_frames[i % len(d_frames)])
                    if per_frame:
                        ms = slots[i % ring]                 # (slot i % ring is on stream i % streams every time: ring = 2 * streams)
                        ms.mask, ms.colours = d_maps[i % len(d_maps)], True
                        z = t_device(z, i, ms)
                    else:
                        z = t_static(z, i)
                    outs[i % ring] = net.inverse_u8(z)
        loop(args.warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        loop(n)
        for st in streams:
            torch.cuda.current_stream().wait_stream(st)
        e1.record()
        e1.synchronize()
        return n / (e0.elapsed_time(e1) * 1e-3)

    rec = {"what": "masked photorealistic video path, one label map per frame vs one map per clip", "size": f"{W}x{H}",
           "labels": K, "precision": args.precision, "streams": args.streams, "frames": args.frames,
           "device": torch.cuda.get_device_name(0)}
    if "a" in args.only:
        rec["a_static_pipeline_fps"] = round(pipeline_rate(t_static, args.frames, False)[0], 2)
        rec["a_static_resident_fps"] = round(resident_rate(False, args.frames), 2)
    if "b" in args.only:
        fps, redo = pipeline_rate(t_device, args.frames, True)
        rec["b_device_pipeline_fps"], rec["b_redo_frames"] = round(fps, 2), redo
        rec["b_device_resident_fps"] = round(resident_rate(True, args.frames), 2)
    if "c" in args.only:
        rec["c_host_pipeline_fps"] = round(pipeline_rate(t_host, args.host_frames, False)[0], 2)
        rec["c_host_frames"] = args.host_frames
    if "a" in args.only and "b" in args.only:
        rec["b_over_a_pipeline"] = round(rec["b_device_pipeline_fps"] / rec["a_static_pipeline_fps"], 4)
        rec["b_over_a_resident"] = round(rec["b_device_resident_fps"] / rec["a_static_resident_fps"], 4)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
