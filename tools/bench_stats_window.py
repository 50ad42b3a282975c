#!/usr/bin/env python
"""The statistics window, measured: the frame rate of the 1080p photorealistic video loop (FramePipeline, synthetic weights,
uint8 frames in and out, bf16x3, depth 4, 3 streams, the style reduced and prefactored once), unmasked and with a 5-label static
mask, at --stats_window 1 (today's route: no ring, no new launch) and at --stats_window 4; then vst_cwct_stats_pool alone.
Writes profiles/stats_window.json and prints it.

    python tools/bench_stats_window.py [--out profiles/stats_window.json] [--frames 48] [--warmup 8] [--parent DIR]
    python tools/bench_stats_window.py --by_label [--out profiles/stats_window_keyed.json]

--by_label: the same loop with a label map per frame (the packed masked route under per-frame plans) at W = 1 and at W = 4 with
FramePipeline(stats_by_label=True); the W = 4 rate is compared with the W = 1 rate of the same run.

Loop timing: wall time around `frames` frames (sink: a no-op) after `warmup` frames; W = 1 and W = 4 alternate three times each
inside one process, so that they share whatever else the host is doing and their spread is known: the median, the batches and
the spread (max - min of the batches of one configuration, the larger of the two).  Every process measures in a fresh child, so
that --parent DIR (a built checkout of the parent commit: its W = 1 is the same code path) is measured the same way, the two
trees alternating twice each.  Kernel timing: HIP events around 50 launches queued behind a long kernel, so that they run back
to back: kernel plus dispatch gap, not the host's enqueue rate.  Clocks are not pinned: compare the rows of one run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_rates(a, windows):
    """{route: {W: [frames/s per batch]}} of the tree on sys.path"""
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict, synthetic_frames, synthetic_mask
    H, W, n = 1080, 1920, a.frames
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234, 16, 2))
    net = net.cuda().eval()
    cw = cWCT()
    frames = [(synthetic_frames(1, H, W, seed=i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(4)]
    with torch.no_grad():
        z_s = net.forward_u8((synthetic_frames(1, 720, 1280, seed=50)[0].permute(1, 2, 0) * 255).byte()[None].cuda())
        s_stats = cw.style_stats(z_s)
        plan = cw.plan_masks(synthetic_mask(H, W, labels=5, seed=3)[None], synthetic_mask(720, 1280, labels=5, seed=4)[None],
                             (1, 32, H, W), tuple(z_s.shape), "cuda")
        plan = cw.bind_style(cw.learn_slots(plan), z_s)
    routes = {"unmasked": (lambda z, i, **k: cw.transfer_with_stats(z, s_stats, **k), None),
              "static_mask_5_labels": (lambda z, i, **k: cw.transfer_with_plan(z, None, plan, **k), plan)}
    runs = []
    for route, (tr, pl) in routes.items():
        for w in windows:
            kw = {} if w == 1 else dict(stats_window=w, frame_stats=lambda z, out=None, pl=pl: cw.frame_stats(z, pl, out=out))
            runs.append((route, w, FramePipeline(net, tr, H, W, depth=4, compute_streams=3, **kw)))

    def go(pipe, count):
        pipe.run((frames[i % 4] for i in range(count)), lambda i, f: None)
        torch.cuda.synchronize()
    for _, _, pipe in runs:
        go(pipe, a.warmup)
    out = {route: {w: [] for w in windows} for route in routes}
    for _ in range(3):
        for route, w, pipe in runs:
            t0 = time.perf_counter()
            go(pipe, n)
            out[route][w].append(round(n / (time.perf_counter() - t0), 2))
    return out


def loop_rates_by_label(a, windows):
    """{route: {W: [frames/s per batch]}} under per-frame label maps: every frame brings its own map (four maps of 4..6 labels
    in turn, so a label's slot moves from frame to frame); W = 1 is the per-frame masked route, W > 1 the window by label"""
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict, synthetic_frames, synthetic_mask
    H, W, n = 1080, 1920, a.frames
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234, 16, 2))
    net = net.cuda().eval()
    cw = cWCT()
    frames = [(synthetic_frames(1, H, W, seed=i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(4)]
    maps = [synthetic_mask(H, W, labels=k, seed=3 + j) for j, k in enumerate((5, 4, 6, 5))]
    maps[1] = np.where(maps[1] == 1, 2, maps[1]).astype(np.uint8)          # label 1 is absent from every fourth frame
    with torch.no_grad():
        z_s = net.forward_u8((synthetic_frames(1, 720, 1280, seed=50)[0].permute(1, 2, 0) * 255).byte()[None].cuda())
        binding = cw.bind_style_labels(z_s, synthetic_mask(720, 1280, labels=6, seed=4))

    def transform(z_c, i, ms, content_stats=None):
        buf = ms.state.get("buffers")
        if buf is None:
            buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, "cuda")
        plan = cw.plan_frame(ms.mask, binding, max_slots=8, buffers=buf, flags=ms.flags)
        kw = {} if content_stats is None else dict(content_stats=content_stats, by_label=True)
        return cw.transfer_with_plan(z_c, None, plan, **kw)
    runs = [(w, FramePipeline(net, transform, H, W, depth=4, compute_streams=3,
                              **({} if w == 1 else dict(stats_window=w, stats_by_label=True)))) for w in windows]

    def go(pipe, count):
        pipe.run((frames[i % 4] for i in range(count)), lambda i, f: None, masks=(maps[i % 4] for i in range(count)))
        torch.cuda.synchronize()
        if pipe.redo_count:
            raise SystemExit("a frame overflowed the packed route: the loop measured something else")
    for _, pipe in runs:
        go(pipe, a.warmup)
    out = {"per_frame_maps": {w: [] for w in windows}}
    pooled = {}
    for _ in range(3):
        for w, pipe in runs:
            t0 = time.perf_counter()
            go(pipe, n)
            out["per_frame_maps"][w].append(round(n / (time.perf_counter() - t0), 2))
            if w > 1:
                pooled[w] = round(pipe.pooled_frames / max(1, pipe.pooled_labels), 3)
    out["frames_pooled_per_live_label"] = pooled
    return out


def kernel_times(reps=50):
    import torch
    from vstnet_amd.cwct import cWCT
    big = torch.empty((8192, 8192), device="cuda").normal_()
    out = []
    for N, R, ages, cut in ((32, 1, 4, 0.0), (32, 1, 4, 0.01), (32, 32, 4, 0.0), (128, 1, 4, 0.0), (32, 1, 8, 0.0), (256, 1, 8, 0.01)):
        rec = 1 + N + N * N
        g = torch.Generator().manual_seed(N + R)
        recs = []
        for _ in range(ages):                   # records of one scene: n = 2e6 pixels, a mean, an SPD covariance
            m = torch.randn(R, N, N, generator=g, dtype=torch.float64)
            r = torch.cat([torch.full((R, 1), 2.0e6, dtype=torch.float64), torch.randn(R, N, generator=g, dtype=torch.float64),
                           (m @ m.transpose(1, 2) / N + torch.eye(N, dtype=torch.float64)).reshape(R, N * N)], dim=1)
            recs.append(r.cuda())
        dst, used = torch.empty_like(recs[0]), torch.zeros(R, dtype=torch.int32, device="cuda")
        fn = lambda: cWCT.pool_stats(recs, decay=0.8, cut=cut, out=dst, used=used)      # noqa: E731
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            torch.mm(big, big)                  # a backlog: the launches below queue up behind it and run back to back
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        row = {"N": N, "records": R, "ages": ages, "cut": cut, "used": int(used[0]), "us": round(e0.elapsed_time(e1) * 1000.0 / reps, 2),
               "bytes_read": ages * R * rec * 8}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def child(a):
    """One measurement in a fresh process: the tree is a.tree."""
    sys.path.insert(0, a.tree)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stats_window.py measures on the GPU; there is none here")
    windows = [int(w) for w in a.windows.split(",")]
    if a.by_label:
        res = {"tree": a.child, "device": torch.cuda.get_device_name(0), "loop": loop_rates_by_label(a, windows)}
        print("RESULT " + json.dumps(res), flush=True)
        return
    res = {"tree": a.child, "loop": loop_rates(a, windows)}
    if a.kernels:
        res["device"] = torch.cuda.get_device_name(0)
        res["pool_kernel"] = kernel_times()
    print("RESULT " + json.dumps(res), flush=True)


def by_label(a):
    """--by_label: one fresh child, W = 1 and W = 4 alternating three times; the W = 4 rate against the W = 1 rate of the same run"""
    out = a.out or os.path.join(REPO, "profiles", "stats_window_keyed.json")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "this", "--tree", REPO, "--windows", "1,4", "--frames",
           str(a.frames), "--warmup", str(a.warmup), "--by_label"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"the measurement failed ({r.returncode}):\n{r.stderr[-3000:]}")
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    b1, b4 = got["loop"]["per_frame_maps"]["1"], got["loop"]["per_frame_maps"]["4"]
    res = {"what": "statistics window by label: the 1080p photorealistic video loop (bf16x3, depth 4, 3 streams) with a label map "
                   "per frame (4..6 labels, packed masked route) at W = 1 (the per-frame route) and W = 4 (stats_by_label: one "
                   "keyed pool launch and one plan copy more per frame)",
           "device": got.get("device"), "frames_per_batch": a.frames,
           "clock_caveat": "clocks not pinned, short runs: compare the rows of this file with each other, not with other files",
           "w1_fps": round(float(np.median(b1)), 2), "w1_fps_batches": b1, "w4_fps": round(float(np.median(b4)), 2),
           "w4_fps_batches": b4, "w4_over_w1": round(float(np.median(b4)) / float(np.median(b1)), 4),
           "spread_fps": round(max(max(b1) - min(b1), max(b4) - min(b4)), 2),
           "frames_pooled_per_live_label": got["loop"]["frames_pooled_per_live_label"]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    print(json.dumps({"written": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its W = 1 rate, measured alternately")
    ap.add_argument("--by_label", action="store_true", help="the loop with a label map per frame at W = 1 and W = 4 "
                    "(FramePipeline(stats_by_label=True)); writes profiles/stats_window_keyed.json")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    ap.add_argument("--windows", default="1,4", help=argparse.SUPPRESS)
    ap.add_argument("--kernels", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)

    def measure(name, tree, windows, kernels=False):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--tree", tree, "--windows", windows, "--frames",
               str(a.frames), "--warmup", str(a.warmup)] + (["--kernels"] if kernels else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"the measurement of {name} failed ({r.returncode}):\n{r.stderr[-3000:]}")
        got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(json.dumps({"tree": name, "loop": got["loop"]}), flush=True)
        return got
    if a.by_label:
        return by_label(a)
    runs = [measure("this", REPO, "1,4", kernels=True)]
    if a.parent is not None:
        runs += [measure("parent", a.parent, "1"), measure("this", REPO, "1,4"), measure("parent", a.parent, "1")]
    res = {"what": "statistics window: the 1080p photorealistic video loop (bf16x3, depth 4, 3 streams) at --stats_window 1 and 4, "
                   "unmasked and with a 5-label static mask; vst_cwct_stats_pool alone (HIP events, launches back to back)",
           "device": runs[0].get("device"), "frames_per_batch": a.frames,
           "clock_caveat": "clocks not pinned, short runs: compare the rows of this file with each other, not with other files",
           "loop": {}, "pool_kernel": runs[0]["pool_kernel"]}
    for route in runs[0]["loop"]:
        row = {}
        for tree in ("this", "parent"):
            for w in ("1", "4"):
                b = [v for r in runs if r["tree"] == tree for v in r["loop"][route].get(w, [])]
                if b:
                    row[f"{tree}_w{w}_fps"] = round(float(np.median(b)), 2)
                    row[f"{tree}_w{w}_fps_batches"] = b
        row["spread_fps"] = round(max(max(v) - min(v) for k, v in row.items() if k.endswith("_batches")), 2)
        res["loop"][route] = row
    out = a.out or os.path.join(REPO, "profiles", "stats_window.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    print(json.dumps({"written": out}))


if __name__ == "__main__":
    main()
