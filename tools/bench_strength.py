#!/usr/bin/env python
"""Strength maps, measured: the frame rate of the video loop (FramePipeline, synthetic photorealistic weights, uint8 frames in
and out, the style reduced once) at 1024 x 1024 without a map and with one static map bound once (cWCT.bind_strength).  Without
a map the loop launches the plain instantiations of the apply kernels, the code the parent commit runs; with a map the BLEND
instantiations read one more float per 128-byte row.  Prints one JSON line.

    python tools/bench_strength.py [--height 1024] [--width 1024] [--frames 48] [--warmup 8] [--streams 3] [--map both|none|static]

Timing: wall time around `frames` frames through the loop (sink included: a no-op) after `warmup` frames; five such batches per
configuration, their median and their spread (min, max).  --map none passes no `strength` argument at all, so the tool also runs
on a tree that predates strength maps (the parent's rate)."""
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


if __name__ == "__main__":
    main()
