#!/usr/bin/env python
"""Whole-frame vs halo-tiled stylisation throughput (vstnet_amd/tiled.py): Mpx/s of an 8192 x 8192 frame whole and in tiles of
4096 and 2048, a 16384 x 16384 frame in tiles of 4096, and the peak device memory of each run.  Photorealistic, bf16x3,
synthetic weights, a 1024 x 1024 style; host uint8 frames in and out (the tiled driver's contract), so the times include the
per-window uploads and downloads.  Prints one JSON line.

    python tools/bench_tiled.py [--repeat 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frame(H, W, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 192, size=(H // 64 + 1, W // 64 + 1, 3), dtype=np.uint8)
    return np.repeat(np.repeat(base, 64, axis=0)[:H], 64, axis=1)[:, :W] + rng.integers(0, 64, size=(H, W, 3), dtype=np.uint8)


def timed(fn, repeat):
    fn()                                         # warm-up (weights packed, workspaces allocated)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    best = float("inf")
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best, torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd import tiled
    from vstnet_amd.synth import synthetic_state_dict
    net = RevResNet(hidden_dim=16, sp_steps=2, precision="bf16x3")
    net.load_state_dict(synthetic_state_dict(1234))
    net = net.cuda().eval()
    cw = cWCT(precision="bf16x3")
    style = frame(1024, 1024, 2)
    r_f, r_i = tiled.receptive_radius(net, "forward"), tiled.receptive_radius(net, "inverse")
    rows = {}
    big = frame(8192, 8192, 1)
    runs = [("8192_whole", big, None), ("8192_tile4096", big, 4096), ("8192_tile2048", big, 2048)]
    for name, img, tile in runs:
        fn = (lambda img=img: tiled.stylize_whole(net, cw, img, style)) if tile is None else \
             (lambda img=img, tile=tile: tiled.stylize_tiled(net, cw, img, style, tile=tile))
        s, peak = timed(fn, args.repeat)
        rows[name] = {"s": round(s, 3), "Mpx_per_s": round(img.shape[0] * img.shape[1] / s / 1e6, 1),
                      "peak_GiB": round(peak / 2 ** 30, 2)}
        torch.cuda.empty_cache()
    del big
    huge = frame(16384, 16384, 3)
    s, peak = timed(lambda: tiled.stylize_tiled(net, cw, huge, style, tile=4096), 1)
    rows["16384_tile4096"] = {"s": round(s, 3), "Mpx_per_s": round(16384 * 16384 / s / 1e6, 1), "peak_GiB": round(peak / 2 ** 30, 2)}
    whole = rows["8192_whole"]["Mpx_per_s"]
    for k, v in rows.items():
        v["work_vs_whole"] = round(whole / v["Mpx_per_s"], 3)
    # halo-area model: pass S + pass 1 (halo r_f) + pass 2 (halo r_f + r_i, encode + decode) over the interior area
    def model(H, tile):
        p1 = sum(np.prod(t.window_hw) for t in tiled.tile_plan(H, H, tile, r_f)) / H / H
        p2 = sum(np.prod(t.window_hw) for t in tiled.tile_plan(H, H, tile, r_f + r_i)) / H / H
        return round((p1 + 2 * p2) / 2, 3)       # whole frame: one encode + one decode of the content
    print(json.dumps({"metric": "tiled stylisation Mpx/s", "radius": [r_f, r_i], "runs": rows,
                      "halo_model_work": {"8192_tile4096": model(8192, 4096), "8192_tile2048": model(8192, 2048),
                                          "16384_tile4096": model(16384, 4096)}}))


if __name__ == "__main__":
    main()
