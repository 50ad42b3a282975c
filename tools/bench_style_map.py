#!/usr/bin/env python
"""Style maps, measured: the frame rate of the 1080p photorealistic video loop (FramePipeline, synthetic weights, uint8 frames
in and out, two styles reduced and prefactored once) with the uniform mix `--alpha_s 0.5 0.5` - the existing route, one factor
launch of two styles and the plain apply in the decode, which the parent commit also has - against a left-to-right gradient
style map bound once (cWCT.bind_style_map): two factor launches per frame and the mix apply in the decode.  Then the two apply
kernels alone, plain (vst_cwct_apply_code) against mix (vst_cwct_apply_code_mix, K = 2; for rows of 32 also K = 4 and 8), at
1920 x 1080 and 1024 x 1024.  Writes profiles/style_map.json and prints it.

    python tools/bench_style_map.py [--out profiles/style_map.json] [--frames 48] [--warmup 8] [--streams 3] [--skip-loop]

--per_frame measures the style map per frame instead ("Style maps per frame"): the same 1080p loop with
K = 2 planes per frame (FramePipeline(style_planes=2): the planes' upload, vst_style_frame, the mix apply) against the loop with
the same map bound once, alternating in one session; and vst_style_frame alone at K = 2 and K = 8 for both sp_steps against the
floor of its bytes, K H W read plus 2 K 4 cH cW written.  Writes profiles/style_map_frames.json.

    python tools/bench_style_map.py --per_frame [--out profiles/style_map_frames.json] [--frames 48] [--warmup 8] [--streams 3]

Loop timing: wall time around `frames` frames (sink: a no-op) after `warmup` frames; five batches per configuration, alternating
so that they share whatever else the host is doing; the median and the batches.  Kernel timing: HIP events around 50 launches
that were queued behind a long kernel, so that they run back to back: kernel plus dispatch gap, not the host's enqueue rate;
bytes = the code read once and written once plus the K weight planes.  Clocks are not pinned: compare the rows of one run."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def gradient_weights(K, cH, cW):
    """K planes: style k peaks at column k (cW - 1) / (K - 1) and fades linearly to its neighbours; exact one-hot columns at
    the peaks, two styles mixed everywhere else; the planes sum to 1"""
    x = np.linspace(0.0, K - 1.0, cW, dtype=np.float64)
    w = np.stack([np.clip(1.0 - np.abs(x - k), 0.0, 1.0) for k in range(K)])
    w = (w / w.sum(axis=0)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(w[:, None, :], (K, cH, cW)))


def loop_rates(a, res):
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict, synthetic_frames
    H, W, n = 1080, 1920, a.frames
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234, 16, 2))
    net = net.cuda().eval()
    cw = cWCT()
    frames = [(synthetic_frames(1, H, W, seed=i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(4)]
    with torch.no_grad():
        stats = [cw.style_stats(net.forward_u8((synthetic_frames(1, 720, 1280, seed=50 + k)[0].permute(1, 2, 0) * 255).byte()[None].cuda()))
                 for k in range(2)]
    bound = cw.bind_style_map(gradient_weights(2, H, W), (1, 32, H, W), "cuda")
    runs = [("uniform_alpha_s", FramePipeline(net, lambda z, i: cw.transfer_with_stats(z, stats, 0.0, alpha_s=[0.5, 0.5]), H, W,
                                              compute_streams=a.streams)),
            ("gradient_style_map", FramePipeline(net, lambda z, i, style_map=None: cw.transfer_with_stats(z, stats, 0.0, style_map=style_map),
                                                 H, W, compute_streams=a.streams, style_map=bound))]

    def go(pipe, count):
        pipe.run((frames[i % 4] for i in range(count)), lambda i, f: None)
        torch.cuda.synchronize()
    for _, pipe in runs:
        go(pipe, a.warmup)
    batches = {key: [] for key, _ in runs}
    for _ in range(5):
        for key, pipe in runs:
            t0 = time.perf_counter()
            go(pipe, n)
            batches[key].append(n / (time.perf_counter() - t0))
    res["loop"] = {"frame": f"{W}x{H}", "frames_per_batch": n, "streams": a.streams}
    for key, b in batches.items():
        res["loop"][key + "_fps"] = round(float(np.median(b)), 2)
        res["loop"][key + "_fps_batches"] = [round(v, 2) for v in b]


def gradient_planes(K, H, W, shift=0):
    """gradient_weights as K 8-bit planes at the frame's size, rolled by `shift` columns: what a frame of a clip brings"""
    w = np.rint(gradient_weights(K, H, W) * 255.0).astype(np.uint8)
    return np.ascontiguousarray(np.roll(w, shift, axis=2))


def per_frame_loop(a, res):
    """the 1080p loop with two planes per frame against the same loop with frame 0's map bound once, alternating"""
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from utils.utils import style_map_weights
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict, synthetic_frames
    H, W, n = 1080, 1920, a.frames
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234, 16, 2))
    net = net.cuda().eval()
    cw = cWCT()
    frames = [(synthetic_frames(1, H, W, seed=i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(4)]
    planes = [gradient_planes(2, H, W, 64 * i) for i in range(4)]
    with torch.no_grad():
        stats = [cw.style_stats(net.forward_u8((synthetic_frames(1, 720, 1280, seed=50 + k)[0].permute(1, 2, 0) * 255).byte()[None].cuda()))
                 for k in range(2)]
    bound = cw.bind_style_map(style_map_weights(list(planes[0])), (1, 32, H, W), "cuda")
    tf = lambda z, i, style_map=None: cw.transfer_with_stats(z, stats, 0.0, style_map=style_map)      # noqa: E731
    static = FramePipeline(net, tf, H, W, compute_streams=a.streams, style_map=bound)
    moving = FramePipeline(net, tf, H, W, compute_streams=a.streams, style_planes=2)

    def go(key, count):
        kw = dict(style_maps=(planes[i % 4] for i in range(count))) if key == "per_frame" else {}
        (moving if key == "per_frame" else static).run((frames[i % 4] for i in range(count)), lambda i, f: None, **kw)
        torch.cuda.synchronize()
    keys = ("static_style_map", "per_frame")
    for key in keys:
        go(key, a.warmup)
    batches = {key: [] for key in keys}
    for _ in range(5):
        for key in keys:
            t0 = time.perf_counter()
            go(key, n)
            batches[key].append(n / (time.perf_counter() - t0))
    loop = {"frame": f"{W}x{H}", "frames_per_batch": n, "streams": a.streams, "planes_per_frame": 2,
            "uploaded_bytes_per_frame": {"frame": 3 * H * W, "planes": 2 * H * W}}
    for key, b in batches.items():
        loop[key + "_fps"] = round(float(np.median(b)), 2)
        loop[key + "_fps_batches"] = [round(v, 2) for v in b]
    ratios = [p / s for p, s in zip(batches["per_frame"], batches["static_style_map"])]
    loop["per_frame_over_static"] = round(float(np.median(batches["per_frame"]) / np.median(batches["static_style_map"])), 4)
    loop["per_frame_over_static_batches"] = [round(v, 4) for v in ratios]
    # the run's own spread: how far the batches of ONE configuration lie apart, relative to their median
    loop["spread"] = {key: round(float((max(b) - min(b)) / np.median(b)), 4) for key, b in batches.items()}
    res["loop"] = loop


def style_frame_times(res, reps=50):
    """vst_style_frame alone, launches back to back (HIP events), against the floor of its bytes"""
    import ctypes as C
    import torch
    from vstnet_amd import _lib
    L = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    big = torch.empty((8192, 8192), device="cuda").normal_()
    H, W = 1080, 1920
    out = []
    for sp in (2, 1):
        n = H * W if sp == 2 else H * W // 4
        for K in (2, 8):
            planes = torch.from_numpy(gradient_planes(K, H, W)).cuda()
            dense = torch.empty((K, n), device="cuda")
            rows = torch.empty((K, n), device="cuda")
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            fn = lambda: _lib.check(L.vst_style_frame(ptr(planes), K, ptr(dense), ptr(rows), ptr(flag), H, W, sp, st()),      # noqa: E731
                                    "vst_style_frame")
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            assert int(flag.item()) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(2):
                torch.mm(big, big)          # a backlog: the launches below queue up behind it and run back to back
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1000.0 / reps
            nbytes = K * H * W + 2 * K * 4 * n
            rec = {"frame": f"{W}x{H}", "sp_steps": sp, "kernel": "vst_style_frame", "K": K, "us": round(us, 1), "bytes": nbytes,
                   "gbytes_per_s": round(nbytes / us / 1e3, 1)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    res["kernels"] = out


def kernel_times(res, reps=50):
    import ctypes as C
    import torch
    from vstnet_amd import _lib
    L = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    big = torch.empty((8192, 8192), device="cuda").normal_()
    out = []
    for (W, H) in ((1920, 1080), (1024, 1024)):
        for sp, N, Ks in ((2, 32, (2, 4, 8)), (1, 128, (2,))):
            rows = H * W if sp == 2 else H * W // 4
            g = torch.Generator().manual_seed(W + sp)
            code = torch.randn(rows * N, generator=g).cuda()
            dst = torch.empty_like(code)
            cH, cW = (H, W) if sp == 2 else (H // 2, W // 2)
            configs = [("plain", 1, None)] + [("mix", K, None) for K in Ks] + [("mix + strength", 2, torch.rand(rows, generator=g).cuda())]
            for name, K, s in configs:
                aff = (torch.randn(K, N * N + N, generator=g) * 0.1).cuda()
                wr = None
                if name != "plain":
                    dense = torch.from_numpy(gradient_weights(K, cH, cW)).cuda()
                    wr = torch.empty_like(dense)
                    for k in range(K):
                        _lib.check(L.vst_map_to_code(ptr(dense[k]), ptr(wr[k]), H, W, sp, st()), "vst_map_to_code")
                if name == "plain":
                    fn = lambda: _lib.check(L.vst_cwct_apply_code(ptr(code), ptr(dst), H, W, sp, ptr(aff), st()), "apply")      # noqa: E731
                else:
                    fn = lambda: _lib.check(L.vst_cwct_apply_code_mix(ptr(code), ptr(dst), H, W, sp, ptr(aff), K, ptr(wr), ptr(s), st()),      # noqa: E731
                                            "apply_mix")
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(2):
                    torch.mm(big, big)          # a backlog: the launches below queue up behind it and run back to back
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                us = e0.elapsed_time(e1) * 1000.0 / reps
                nbytes = 2 * rows * N * 4 + (0 if name == "plain" else K * rows * 4) + (rows * 4 if s is not None else 0)
                rec = {"frame": f"{W}x{H}", "rows_of": N, "kernel": name, "K": K, "us": round(us, 1), "bytes": nbytes,
                       "gbytes_per_s": round(nbytes / us / 1e3, 1)}
                print(json.dumps(rec), flush=True)
                out.append(rec)
    res["kernels"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--per_frame", action="store_true", help="the style map per frame against the static map, and vst_style_frame")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    a.out = a.out or os.path.join(REPO, "profiles", "style_map_frames.json" if a.per_frame else "style_map.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_style_map.py measures on the GPU; there is none here")
    res = {"what": "style maps: the 1080p photorealistic video loop with two bound styles, uniform --alpha_s against a gradient "
                   "style map; the plain and the mix apply kernels alone (HIP events, launches back to back)",
           "device": torch.cuda.get_device_name(0),
           "clock_caveat": "clocks not pinned, one short run: compare the rows of this file with each other, not with other files"}
    if a.per_frame:
        res["what"] = ("style maps per frame: the 1080p photorealistic video loop with two 8-bit planes per frame (upload, "
                       "vst_style_frame, mix apply) against the same loop with the map bound once; vst_style_frame alone (HIP "
                       "events, launches back to back) against the floor of its bytes, K H W read + 2 K 4 cH cW written")
        if not a.skip_loop:
            per_frame_loop(a, res)
            print(json.dumps(res["loop"]), flush=True)
        style_frame_times(res)
    else:
        if not a.skip_loop:
            loop_rates(a, res)
            print(json.dumps(res["loop"]), flush=True)
        kernel_times(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
