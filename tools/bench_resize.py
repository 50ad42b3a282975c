"""The device resize measured (vstnet_amd/resize.py, csrc/resize.hip): kernel times of every pass, and video_transfer.py end to
end with --resize host and --resize device.

    python tools/bench_resize.py [--out profiles/device_resize.json] [--frames 300] [--runs 3] [--skip-e2e]
                                 [--compare-tree DIR]

Kernel times: HIP events around `--launches` back-to-back launches of one pass after a warm-up, per pass of the two img_resize
steps and of the resize to the writer size, at 1920x1080 and 3840x2160 sources with --max_size 1280; bytes = what the pass must
read and write once (source rows + result), so bytes/s is the algorithmic rate, not the cache traffic.  Clocks are whatever the
card runs at under this short load: the numbers are for comparing passes and for judging them against a frame's milliseconds,
not shares of peak.
End to end: a 1080p JPEG clip through video_transfer.main (files in, numbered PNGs out) - one child process per mode, one
warm-up run and `--runs` timed runs in it -, and the CPU seconds a decode worker spends per frame (decode alone, decode +
img_resize; thread CPU time, one thread).  --compare-tree DIR runs the host mode in another checkout of this repository as
well (the parent commit: the default path must not move).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def time_launches(fn, launches, warmup=10):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches


def kernel_times(launches):
    import torch
    from vstnet_amd.resize import resize_u8, resize_to_u8, img_resize_steps
    out = []
    for (W, H) in ((1920, 1080), (3840, 2160)):
        g = torch.Generator().manual_seed(W)
        cur = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).cuda()
        for n, (tw, th) in enumerate(img_resize_steps((W, H), 1280, 4)):
            h, w = int(cur.shape[0]), int(cur.shape[1])
            mid = torch.empty((h, tw, 3), dtype=torch.uint8, device="cuda")
            dst = torch.empty((th, tw, 3), dtype=torch.uint8, device="cuda")
            for name, src, d, wh in (("horizontal", cur, mid, (tw, h)), ("vertical", mid, dst, (tw, th))):
                sh, sw = int(src.shape[0]), int(src.shape[1])
                if (sw, sh) == wh:
                    out.append({"source": f"{W}x{H}", "pass": f"u8 step {n + 1} {name}", "shape": f"{sw}x{sh} -> {wh[0]}x{wh[1]}",
                                "skipped": "size unchanged"})
                    continue
                sec = time_launches(lambda: resize_u8(src, wh, out=d), launches)
                nbytes = 3 * (sh * sw + wh[0] * wh[1])
                out.append({"source": f"{W}x{H}", "pass": f"u8 step {n + 1} {name}", "shape": f"{sw}x{sh} -> {wh[0]}x{wh[1]}",
                            "us": round(sec * 1e6, 2), "bytes": nbytes, "gbytes_per_s": round(nbytes / sec / 1e9, 1)})
            cur = dst
        # the writer-size quirk: the clip is written at 1280 x <source height> while it is stylised at 1280x720
        sh, sw = int(cur.shape[0]), int(cur.shape[1])
        x = torch.rand((1, 3, sh, sw), generator=g).cuda()
        dst = torch.empty((1, H, sw, 3), dtype=torch.uint8, device="cuda")
        sec = time_launches(lambda: resize_to_u8(x, (H, sw), out=dst), launches)
        nbytes = 4 * 3 * sh * sw + 3 * H * sw
        out.append({"source": f"{W}x{H}", "pass": "output f32 -> u8 (vertical only: the width is the writer's)",
                    "shape": f"{sw}x{sh} -> {sw}x{H}", "us": round(sec * 1e6, 2), "bytes": nbytes,
                    "gbytes_per_s": round(nbytes / sec / 1e9, 1)})
        dst = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda")
        tmp = torch.empty(3 * sh * W, dtype=torch.float32, device="cuda")
        sec = time_launches(lambda: resize_to_u8(x, (H, W), out=dst, tmp=tmp), launches)
        nbytes = 4 * 3 * sh * sw + 2 * 4 * 3 * sh * W + 3 * H * W
        out.append({"source": f"{W}x{H}", "pass": "output f32 -> u8 (both passes, back to the source size)",
                    "shape": f"{sw}x{sh} -> {W}x{H}", "us": round(sec * 1e6, 2), "bytes": nbytes,
                    "gbytes_per_s": round(nbytes / sec / 1e9, 1)})
    return out


def make_clip(d, frames, H=1080, W=1920):
    from PIL import Image
    from tools.video_e2e import natural_frame
    clip = os.path.join(d, "clip")
    os.makedirs(clip)
    first = []
    for t in range(8):                                          # 8 distinct frames, cycled
        p = os.path.join(clip, "%04d.jpg" % t)
        Image.fromarray(natural_frame(H, W, t, seed=7)).save(p, quality=92)
        first.append(p)
    for i in range(8, frames):
        os.link(first[i % 8], os.path.join(clip, "%04d.jpg" % i))
    Image.fromarray(natural_frame(H, W, 3, seed=11)).save(os.path.join(d, "style.jpg"), quality=92)
    return clip, os.path.join(d, "style.jpg")


def decode_cpu_seconds(clip, max_size, n=16):
    """thread CPU seconds per frame of what a decode worker does: decode alone (--resize device), decode + img_resize (host)"""
    from PIL import Image
    from utils.utils import img_resize
    files = sorted(os.listdir(clip))[:n]
    res = {}
    for name, fn in (("decode", lambda im: np.asarray(im, dtype=np.uint8)),
                     ("decode_img_resize", lambda im: np.asarray(img_resize(im, max_size, down_scale=4), dtype=np.uint8))):
        t0 = time.thread_time()
        for f in files:
            fn(Image.open(os.path.join(clip, f)).convert("RGB"))
        res[name] = round((time.thread_time() - t0) / len(files), 5)
    return res


CHILD = """
import json, os, resource, sys, time
tree, runs, argv = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
sys.path.insert(0, tree)
os.chdir(tree)
import video_transfer
video_transfer.main(argv)                       # warm-up: network build, code objects, ring buffers
out = []
for _ in range(runs):
    r0, t0 = resource.getrusage(resource.RUSAGE_SELF), time.perf_counter()
    d = video_transfer.main(argv)
    dt, r1 = time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_SELF)
    n = len([f for f in os.listdir(d) if f.endswith(".png")])
    out.append({"frames": n, "seconds": round(dt, 3), "frames_per_s": round(n / dt, 2),
                "process_cpu_s_per_frame": round((r1.ru_utime + r1.ru_stime - r0.ru_utime - r0.ru_stime) / n, 5)})
print("E2E " + json.dumps(out), flush=True)
"""


def e2e(tree, mode, clip, style, out_dir, runs):
    argv = ["--video", clip, "--style", style, "--out_dir", out_dir, "--max_size", "1280", "--synthetic_weights", "--frames_only",
            "--depth", "6"] + (["--resize", mode] if mode is not None else [])
    p = subprocess.run([sys.executable, "-c", CHILD, tree, str(runs)] + argv, capture_output=True, text=True, timeout=900,
                       cwd=tree)
    if p.returncode != 0:
        raise RuntimeError(f"end-to-end run failed ({tree}, {mode}):\n{p.stderr[-3000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("E2E ")][-1]
    return json.loads(line[4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_resize.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--compare-tree", default=None, help="another checkout of this repository (built) to run the host mode in")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize.py measures on the GPU; there is none here")
    rec = {"what": "device resize: per-pass kernel times (HIP events, back-to-back launches) and video_transfer.py end to end",
           "device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
           "clock_caveat": "clocks not pinned; short bursts of a small kernel: compare passes, do not read as shares of peak",
           "kernels": kernel_times(args.launches)}
    for k in rec["kernels"]:
        print(json.dumps(k), flush=True)
    if not args.skip_e2e:
        with tempfile.TemporaryDirectory(prefix="vst_resize_") as d:
            clip, style = make_clip(d, args.frames)
            rec["decode_worker_cpu_s_per_frame"] = decode_cpu_seconds(clip, 1280)
            rec["end_to_end"] = {"clip": f"{args.frames} frames 1920x1080 JPEG, --max_size 1280, PNGs out at 1280x1080",
                                 "runs_per_mode": args.runs}
            modes = [("host", REPO, "host"), ("device", REPO, "device")]
            if args.compare_tree:
                modes = [("host_compare_tree", os.path.abspath(args.compare_tree), None)] + modes + \
                        [("host_compare_tree_again", os.path.abspath(args.compare_tree), None), ("host_again", REPO, "host")]
            for name, tree, mode in modes:
                rec["end_to_end"][name] = e2e(tree, mode, clip, style, os.path.join(d, "out_" + name), args.runs)
                print(name, json.dumps(rec["end_to_end"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
