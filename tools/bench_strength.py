#!/usr/bin/env python
"""Strength maps, measured: the frame rate of the video loop (FramePipeline, synthetic photorealistic weights, uint8 frames in
and out, the style reduced once) at 1024 x 1024 without a map and with one static map bound once (cWCT.bind_strength).  Without
a map the loop launches the plain instantiations of the apply kernels, the code the parent commit runs; with a map the BLEND
instantiations read one more float per 128-byte row.  Prints one JSON line.

    python tools/bench_strength.py [--height 1024] [--width 1024] [--frames 48] [--warmup 8] [--streams 3] [--map both|none|static]

Timing: wall time around `frames` frames through the loop (sink included: a no-op) after `warmup` frames; five such batches per
configuration, their median and their spread (min, max).  --map none passes no `strength` argument at all, so the tool also runs
on a tree that predates strength maps (the parent's rate).

--per_frame adds the per-frame maps (cWCT.frame_strength, one vst_strength_frame launch in the frame's stream) next to the static
map: `per_frame_device` makes every frame's map from a matte that is already on the card, `per_frame_upload` is the full loop of
run(..., mattes=...) - pinned copy, upload, launch; with --matte_height / --matte_width the mattes arrive at that size and are
resized on the card as well.  The configurations' batches alternate, so that they share whatever else the host is doing.
`strength_frame_us` is the kernel's own time from HIP events around 200 launches (both outputs) that were queued behind a long
kernel, so that they run back to back: kernel plus dispatch gap, not the host's enqueue rate."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gradient_map(H, W):
    """left to right from 0 to 1, with a band of exact zeros and one of exact ones: every kind of row the kernels meet"""
    m = np.tile(np.linspace(0.0, 1.0, W, dtype=np.float32), (H, 1))
    m[: H // 8] = 0.0
    m[-(H // 8):] = 1.0
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--map", default="both", choices=("both", "none", "static"))
    ap.add_argument("--per_frame", action="store_true")
    ap.add_argument("--matte_height", type=int, default=None)
    ap.add_argument("--matte_width", type=int, default=None)
    a = ap.parse_args()
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict, synthetic_frames
    H, W, n = a.height, a.width, a.frames
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234, 16, 2))
    net = net.cuda().eval()
    cw = cWCT()
    frames = [(synthetic_frames(1, H, W, seed=i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(4)]
    style = (synthetic_frames(1, H, W, seed=50)[0].permute(1, 2, 0) * 255).byte()[None].cuda()
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(style))
    res = {"height": H, "width": W, "frames": n, "streams": a.streams}
    configs = []
    if a.map in ("both", "none"):
        configs.append(("no_map", lambda z, i: cw.transfer_with_stats(z, stats)))
    if a.map in ("both", "static"):
        bound = cw.bind_strength(gradient_map(H, W), (1, 32, H, W), "cuda")
        configs.append(("static_map", lambda z, i: cw.transfer_with_stats(z, stats, strength=bound)))
    if a.per_frame:
        return per_frame(a, res, net, cw, stats, frames, configs)
    for key, tf in configs:
        pipe = FramePipeline(net, tf, H, W, compute_streams=a.streams)
        pipe.run((frames[i % 4] for i in range(a.warmup)), lambda i, f: None)
        torch.cuda.synchronize()
        batches = []
        for _ in range(5):
            t0 = time.perf_counter()
            pipe.run((frames[i % 4] for i in range(n)), lambda i, f: None)
            torch.cuda.synchronize()
            batches.append(n / (time.perf_counter() - t0))
        res[key + "_fps"] = round(float(np.median(batches)), 2)
        res[key + "_fps_batches"] = [round(b, 2) for b in batches]
    print(json.dumps(res))


def per_frame(a, res, net, cw, stats, frames, configs):
    import torch
    from vstnet_amd.pipeline import FramePipeline
    H, W, n = a.height, a.width, a.frames
    shape = (1, 32, H, W)
    rng = np.random.default_rng(0)
    mh, mw = a.matte_height or H, a.matte_width or W
    mattes = [rng.integers(0, 256, (mh, mw), dtype=np.uint8) for _ in range(4)]
    on_card = [torch.from_numpy(rng.integers(0, 256, (H, W), dtype=np.uint8)).cuda() for _ in range(4)]
    depth = 4
    slots = [cw.empty_strength(shape, "cuda") for _ in range(depth)]         # (frame i is the tenant of ring slot i % depth)
    runs = [(key, FramePipeline(net, tf, H, W, compute_streams=a.streams, depth=depth), {}) for key, tf in configs]
    runs.append(("per_frame_device", FramePipeline(
        net, lambda z, i: cw.transfer_with_stats(z, stats, strength=cw.frame_strength(shape, matte=on_card[i % 4], out=slots[i % depth])),
        H, W, compute_streams=a.streams, depth=depth), {}))
    runs.append(("per_frame_upload", FramePipeline(
        net, lambda z, i, strength=None: cw.transfer_with_stats(z, stats, strength=strength), H, W, compute_streams=a.streams,
        depth=depth, matte_hw=(mh, mw)), {"mattes": True}))
    res["matte_hw"] = [mh, mw]

    def go(pipe, kw, count):
        extra = {"mattes": (mattes[i % 4] for i in range(count))} if kw else {}
        pipe.run((frames[i % 4] for i in range(count)), lambda i, f: None, **extra)
        torch.cuda.synchronize()
    for _, pipe, kw in runs:
        go(pipe, kw, a.warmup)
    batches = {key: [] for key, _, _ in runs}
    for _ in range(5):
        for key, pipe, kw in runs:
            t0 = time.perf_counter()
            go(pipe, kw, n)
            batches[key].append(n / (time.perf_counter() - t0))
    for key, b in batches.items():
        res[key + "_fps"] = round(float(np.median(b)), 2)
        res[key + "_fps_batches"] = [round(v, 2) for v in b]
    # the kernel alone: HIP events around back-to-back launches on one stream
    reps = 200
    for _ in range(20):
        cw.frame_strength(shape, matte=on_card[0], out=slots[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    big = torch.empty((8192, 8192), device="cuda").normal_()
    torch.cuda.synchronize()
    for _ in range(3):
        torch.mm(big, big)              # tens of milliseconds of backlog: the launches below queue up behind it, so the
    e0.record()                         # events see kernels back to back, not the host's enqueue rate
    for r in range(reps):
        cw.frame_strength(shape, matte=on_card[r % 4], out=slots[r % depth])
    e1.record()
    e1.synchronize()
    res["strength_frame_us"] = round(e0.elapsed_time(e1) * 1000.0 / reps, 2)
    res["strength_frame_bytes"] = H * W * 9
    res["strength_frame_GBps"] = round(H * W * 9 / (res["strength_frame_us"] * 1e-6) / 1e9, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
