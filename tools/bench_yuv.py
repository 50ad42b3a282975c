"""The raw video edge measured (csrc/yuv.hip vst_yuv_to_rgb_u8 / vst_rgb_to_yuv_u8, FramePipeline(src_yuv=, out_yuv=),
video_transfer.py on .y4m files; DESIGN.md section 6, "Raw video edge").

    python tools/bench_yuv.py [--out profiles/yuv_edge.json] [--frames 300] [--repeats 3] [--samples 7] [--launches 200]

(a) the kernels: HIP events around `--launches` back-to-back calls of the C entry point (through ctypes, arguments made once)
    after a warm-up, `--samples` such windows, median and min / max, at 1920x1080 and 3840x2160 for every layout (BT.709,
    limited range); bytes = what a launch must read and write once (3 per pixel of RGB + 1.5 or 3 of planes), so bytes/s is
    the algorithmic rate beside the streaming bound.  The same call on a 16x16 frame gives the floor of the method - the rate
    at which this host issues launches: a time near the floor says "no slower than that", not how fast the kernel is.
(b) FramePipeline at 1920x1080, host memory to host memory, plain cWCT, a sink that drops the frame: RGB frames in and out
    against 4:2:0 planes in and out; `--frames` frames per window, `--repeats` windows per variant, the variants ALTERNATING
    inside one process.
(c) video_transfer.py end to end, `--frames` frames at 1920x1080 (--max_size 1920): .y4m in -> .y4m out against a JPEG
    directory in -> numbered PNGs out (--resize host, the default, and --resize device), and the JPEG directory -> .y4m out to
    tell the two sides apart; one child process per route, a warm-up run and `--repeats` timed runs each, all in this one
    session, the y4m route first and once more last (drift of the session shows as the difference of the two).  A run's
    output directory is removed before it starts, outside the timing; the seconds inside FramePipeline.run and inside the
    y4m writer's open and close are recorded next to the run's total.
Clocks are not pinned and the card may be shared: read the spread next to every median.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_BYTES_PER_S = 8.0e12        # MI355X HBM3E, vendor peak


def spread(values, digits=2):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits),
            "max": round(max(values), digits), "samples": len(values)}


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


def kernel_times(launches, samples):
    import ctypes as C
    import torch
    from vstnet_amd import _lib
    from vstnet_amd.yuv import YuvSpec
    L, vp = _lib.lib(), C.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    out = []
    for (H, W) in ((16, 16), (1080, 1920), (2160, 3840)):
        g = torch.Generator().manual_seed(H)
        rgb = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).cuda()
        for layout in ("444", "420jpeg", "420mpeg2"):
            spec = YuvSpec(layout, "bt709", "limited")
            flat = torch.randint(0, 256, (spec.frame_bytes(H, W),), dtype=torch.uint8, generator=g).cuda()
            dst_rgb, dst_flat = torch.empty_like(rgb), torch.empty_like(flat)
            lay, mat, rng = spec.codes
            (ys, cs, _), base = spec.plane_shapes(H, W), flat.data_ptr()
            src = [vp(base), vp(base + ys[0] * ys[1]), vp(base + ys[0] * ys[1] + cs[0] * cs[1])]
            base = dst_flat.data_ptr()
            dst = [vp(base), vp(base + ys[0] * ys[1]), vp(base + ys[0] * ys[1] + cs[0] * cs[1])]
            p_rgb, p_dst_rgb = vp(rgb.data_ptr()), vp(dst_rgb.data_ptr())
            for name, fn in (("vst_yuv_to_rgb_u8", lambda: L.vst_yuv_to_rgb_u8(src[0], src[1], src[2], H, W, lay, mat, rng, p_dst_rgb, stream)),
                             ("vst_rgb_to_yuv_u8", lambda: L.vst_rgb_to_yuv_u8(p_rgb, H, W, lay, mat, rng, dst[0], dst[1], dst[2], stream))):
                us = [time_launches(fn, launches) * 1e6 for _ in range(samples)]
                nbytes = 3 * H * W + spec.frame_bytes(H, W)
                med = statistics.median(us)
                out.append({"kernel": name, "frame": f"{W}x{H}" + (" (the method's floor)" if H == 16 else ""), "layout": layout,
                            "us": spread(us), "bytes": nbytes,
                            "gbytes_per_s_at_median": round(nbytes / med / 1e3, 1),
                            "streaming_bound_us": round(nbytes / HBM_PEAK_BYTES_PER_S * 1e6, 2)})
    return out


def pipeline_rates(n_frames, repeats, H=1080, W=1920):
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict
    from vstnet_amd.yuv import YuvSpec, rgb_to_yuv_host
    from tools.video_e2e import natural_frame
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234))
    net = net.to("cuda").eval()
    cw = cWCT()
    spec = YuvSpec("420jpeg", "bt709", "limited")
    distinct = [natural_frame(H, W, t, seed=7) for t in range(4)]
    planes = [rgb_to_yuv_host(f, spec) for f in distinct]
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    kw = dict(depth=4, compute_streams=3)
    runs = {"rgb_in_rgb_out": (FramePipeline(net, tf, H, W, **kw), [distinct[i % 4] for i in range(n_frames)]),
            "yuv420_in_yuv420_out": (FramePipeline(net, tf, H, W, src_yuv=spec, out_yuv=spec, **kw),
                                     [planes[i % 4] for i in range(n_frames)])}
    sink = lambda i, a: None                                                # noqa: E731
    for p, frames in runs.values():         # warm-up: code objects, rings, workspaces of every stream
        p.run(frames[:24], sink)
    torch.cuda.synchronize()
    fps = {k: [] for k in runs}
    for _ in range(repeats):                # the variants alternate: drift of clocks and neighbours hits both alike
        for k, (p, frames) in runs.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink)
            fps[k].append(n / (time.perf_counter() - t0))
    rec = {"frame": f"{W}x{H}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
           "host_bytes_per_frame_each_way": {"rgb_in_rgb_out": 3 * H * W, "yuv420_in_yuv420_out": spec.frame_bytes(H, W)},
           "frames_per_s": {k: spread(v) for k, v in fps.items()}}
    med = {k: statistics.median(v) for k, v in fps.items()}
    rec["ms_per_frame_at_median"] = {k: round(1e3 / v, 3) for k, v in med.items()}
    rec["yuv_over_rgb_at_median"] = round(med["yuv420_in_yuv420_out"] / med["rgb_in_rgb_out"], 4)
    return rec


CHILD = """
import collections, json, os, resource, shutil, sys, time
tree, runs, argv = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
sys.path.insert(0, tree)
os.chdir(tree)
import video_transfer
from vstnet_amd import pipeline, y4m
spent = collections.defaultdict(float)          # wall-clock seconds inside the frame loop and inside the y4m writer's open / close


def clocked(cls, name, key):
    f = getattr(cls, name)

    def g(*a, **k):
        t = time.perf_counter()
        try:
            return f(*a, **k)
        finally:
            spent[key] += time.perf_counter() - t
    setattr(cls, name, g)


clocked(pipeline.FramePipeline, "run", "seconds_in_frame_loop")
clocked(y4m.Y4MWriter, "__init__", "seconds_opening_y4m")
clocked(y4m.Y4MWriter, "close", "seconds_closing_y4m")
out_dir = argv[argv.index("--out_dir") + 1]
video_transfer.main(argv)                       # warm-up: network build, code objects, ring buffers
out = []
for _ in range(runs):
    shutil.rmtree(out_dir, ignore_errors=True)  # (no run pays for truncating the files of the one before it)
    spent.clear()
    r0, t0 = resource.getrusage(resource.RUSAGE_SELF), time.perf_counter()
    video_transfer.main(argv)
    dt, r1 = time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_SELF)
    n = int(os.environ["BENCH_FRAMES"])
    out.append({"frames": n, "seconds": round(dt, 3), "frames_per_s": round(n / dt, 2),
                "process_cpu_s_per_frame": round((r1.ru_utime + r1.ru_stime - r0.ru_utime - r0.ru_stime) / n, 5),
                **{k: round(v, 3) for k, v in sorted(spent.items())}})
print("E2E " + json.dumps(out), flush=True)
"""


def make_clips(d, n_frames, H=1080, W=1920):
    """the same 8 distinct frames, cycled: a JPEG directory and a C420jpeg .y4m file (BT.709, limited range)"""
    from PIL import Image
    from tools.video_e2e import natural_frame
    from vstnet_amd.y4m import Y4MWriter
    from vstnet_amd.yuv import YuvSpec, rgb_to_yuv_host
    spec = YuvSpec("420jpeg", "bt709", "limited")
    clip = os.path.join(d, "clip")
    os.makedirs(clip)
    base = [natural_frame(H, W, t, seed=7) for t in range(8)]
    first = []
    for t, f in enumerate(base):
        p = os.path.join(clip, "%04d.jpg" % t)
        Image.fromarray(f).save(p, quality=92)
        first.append(p)
    for i in range(8, n_frames):
        os.link(first[i % 8], os.path.join(clip, "%04d.jpg" % i))
    planes = [rgb_to_yuv_host(f, spec) for f in base]
    with Y4MWriter(os.path.join(d, "clip.y4m"), W, H, 30, spec) as w:
        for i in range(n_frames):
            w.write(planes[i % 8])
    Image.fromarray(natural_frame(H, W, 3, seed=11)).save(os.path.join(d, "style.jpg"), quality=92)
    return clip, os.path.join(d, "clip.y4m"), os.path.join(d, "style.jpg")


def e2e(video, style, out_dir, n_frames, repeats, extra):
    argv = ["--video", video, "--style", style, "--out_dir", out_dir, "--max_size", "1920", "--synthetic_weights", "--frames_only",
            "--depth", "6"] + extra
    p = subprocess.run([sys.executable, "-c", CHILD, REPO, str(repeats)] + argv, capture_output=True, text=True, timeout=900,
                       cwd=REPO, env=dict(os.environ, BENCH_FRAMES=str(n_frames)))
    if p.returncode != 0:
        raise RuntimeError(f"end-to-end run failed ({video} {extra}):\n{p.stderr[-3000:]}")
    runs = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("E2E ")][-1][4:])
    shutil.rmtree(out_dir, ignore_errors=True)
    return {"runs": runs, "frames_per_s": spread([r["frames_per_s"] for r in runs]),
            "frames_per_s_of_the_frame_loop": spread([r["frames"] / r["seconds_in_frame_loop"] for r in runs]),
            "process_cpu_s_per_frame": spread([r["process_cpu_s_per_frame"] for r in runs], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "yuv_edge.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv.py measures on the GPU; there is none here")
    rec = {"what": "the raw video edge: (a) kernel times per layout, (b) FramePipeline RGB against 4:2:0 planes both ways, "
                   "(c) video_transfer.py y4m -> y4m against JPEG directory -> PNGs",
           "device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
           "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
           "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "kernels": kernel_times(args.launches, args.samples)}
    for k in rec["kernels"]:
        print(json.dumps(k), flush=True)
    if not args.skip_pipeline:
        rec["pipeline_1080p"] = pipeline_rates(args.frames, args.repeats)
        print(json.dumps(rec["pipeline_1080p"]), flush=True)
    if not args.skip_e2e:
        d = tempfile.mkdtemp(prefix="bench_yuv_")
        try:
            clip, y4m, style = make_clips(d, args.frames)
            out = os.path.join(d, "out")
            rec["end_to_end_1080p"] = {
                "clip": f"{args.frames} frames 1920x1080 (8 distinct, cycled), --max_size 1920, --depth 6, synthetic weights",
                "y4m_to_y4m": e2e(y4m, style, out, args.frames, args.repeats, []),
                "jpeg_dir_to_pngs_resize_host": e2e(clip, style, out, args.frames, args.repeats, []),
                "jpeg_dir_to_pngs_resize_device": e2e(clip, style, out, args.frames, args.repeats, ["--resize", "device"]),
                "jpeg_dir_to_y4m": e2e(clip, style, out, args.frames, args.repeats, ["--out_format", "y4m"]),
                "y4m_to_y4m_again": e2e(y4m, style, out, args.frames, args.repeats, [])}
            print(json.dumps(rec["end_to_end_1080p"]), flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
