"""The guided upscale measured (csrc/guided.hip, FramePipeline(upscale="guided"); DESIGN.md section 6, "Guided upscale").

    python tools/bench_guided.py [--out profiles/guided_upscale.json] [--frames 300] [--repeats 3] [--samples 7] [--launches 50]
    rocprofv3 --kernel-trace --stats -d DIR -o guided --output-format csv -- python tools/bench_guided.py --trace-run
    python tools/bench_guided.py --merge-stats DIR/.../guided_kernel_stats.csv [--out profiles/guided_upscale.json]

Workload: a 3840x2160 synthetic clip stylised at --max_size 1280 (working size 1280x720), radius 4, eps 1e-3.
(a) the fit (four launches) and the two apply kernels: HIP events around `--launches` back-to-back calls of the C entry point after
    a warm-up, `--samples` such windows, median and min / max.  For the apply kernels the floor of their frame bytes stands beside
    the time: 6 B x H x W (the source frame read, the result written; 15 B for the f32 form) over the HBM rate measured for
    streaming kernels on this card (6.29 TB/s); the coefficient planes (12 x h x w x 4 B, read four times over through the caches)
    are not in the floor.
(b) FramePipeline, host memory to host memory, plain cWCT, a sink that drops the frame: upscale="guided" (frames leave at
    3840x2160) against the bicubic resize to the writer size the script gives this clip (video_transfer.writer_size), `--frames`
    frames per window, `--repeats` (at least 3) windows per variant, the variants ALTERNATING inside one process, in one session.
(c) once, for context: the whole-frame stylisation at 3840x2160, the route the guided upscale stands in for.
--trace-run makes a few fit + apply calls and nothing else, for a rocprofv3 --kernel-trace --stats run of its own (no counters
in that run); --merge-stats writes that run's per-kernel rows of the guided kernels into the profile file.
Clocks are not pinned and the card may be shared: read the spread next to every median.  The output file keeps the keys it
already has (the float budget tests/test_guided_host.py records there).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.bench_yuv import spread, time_launches  # noqa: E402

HBM_STREAM_BYTES_PER_S = 6.29e12       # measured float4 copy on this card (79 % of the 8.0 TB/s peak)
SRC_HW, MAX_SIZE, RADIUS, EPS = (2160, 3840), 1280, 4, 1e-3


def work_hw():
    from vstnet_amd.resize import img_resize_size
    w, h = img_resize_size((SRC_HW[1], SRC_HW[0]), MAX_SIZE, 4)
    return h, w


def kernel_calls():
    """(name, frame bytes or None, call) of the fit and the two apply forms on random frames of the workload's sizes"""
    import ctypes as C
    import torch
    from vstnet_amd import _lib, guided
    L, vp = _lib.lib(), C.c_void_p
    (h, w), (H, W) = work_hw(), SRC_HW
    g = torch.Generator().manual_seed(1)
    guide = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda()
    target = torch.rand((3, h, w), dtype=torch.float32, generator=g).cuda()
    src = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).cuda()
    coef = torch.empty((12, h, w), dtype=torch.float32, device="cuda")
    ws = torch.empty(guided.workspace_bytes(h, w, RADIUS), dtype=torch.uint8, device="cuda")
    out_u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    out_f32 = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    keep = (guide, target, src, coef, ws, out_u8, out_f32)
    p = [vp(t.data_ptr()) for t in keep]
    calls = (("vst_guided_fit", None, lambda: L.vst_guided_fit(p[0], p[1], h, w, RADIUS, EPS, p[3], p[4], st)),
             ("vst_guided_apply_u8", 6 * H * W, lambda: L.vst_guided_apply_u8(p[3], h, w, p[2], H, W, p[5], st)),
             ("vst_guided_apply_f32", 15 * H * W, lambda: L.vst_guided_apply_f32(p[3], h, w, p[2], H, W, p[6], st)))
    return calls, keep


def kernel_times(launches, samples):
    from vstnet_amd import _lib
    calls, keep = kernel_calls()
    (h, w), (H, W) = work_hw(), SRC_HW
    out = []
    for name, nbytes, fn in calls:
        _lib.check(fn(), name)
        us = [time_launches(fn, launches) * 1e6 for _ in range(samples)]
        row = {"call": name, "working_size": f"{w}x{h}", "full_size": f"{W}x{H}", "radius": RADIUS, "us": spread(us)}
        if nbytes is not None:
            floor = nbytes / HBM_STREAM_BYTES_PER_S * 1e6
            row.update(frame_bytes=nbytes, frame_bytes_floor_us=round(floor, 2),
                       time_over_floor_at_median=round(statistics.median(us) / floor, 2),
                       coefficient_plane_bytes=48 * h * w)
        out.append(row)
    return out


def trace_run(n=20):
    import torch
    from vstnet_amd import _lib
    calls, keep = kernel_calls()
    for _ in range(n):
        for name, _, fn in calls:
            _lib.check(fn(), name)
    torch.cuda.synchronize()


def merge_stats(path, out):
    rows = [r for r in csv.DictReader(open(path)) if "guided_" in r.get("Name", "")]
    keys = ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")
    rec = json.load(open(out)) if os.path.exists(out) else {}
    rec["rocprofv3_kernel_stats"] = {"what": "rocprofv3 --kernel-trace --stats of tools/bench_guided.py --trace-run (no counters)",
                                     "rows": [{k: r.get(k) for k in keys} for r in rows]}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["rocprofv3_kernel_stats"]))


def make_net():
    from models.RevResNet import RevResNet
    from vstnet_amd.synth import synthetic_state_dict
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234))
    return net.to("cuda").eval()


def pipeline_rates(n_frames, repeats):
    import torch
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.resize import resize_to_u8
    from tools.video_e2e import natural_frame
    from video_transfer import writer_size
    net, cw = make_net(), cWCT()
    (h, w), (H, W) = work_hw(), SRC_HW
    wo, ho = writer_size((W, H), MAX_SIZE)
    distinct = [natural_frame(H, W, t, seed=7) for t in range(4)]
    frames = [distinct[i % 4] for i in range(n_frames)]
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    kw = dict(depth=4, compute_streams=3, src_height=H, src_width=W, max_size=MAX_SIZE, down_scale=4)
    bicubic = lambda z: resize_to_u8(net(z, forward=False), (ho, wo))      # noqa: E731  (video_transfer.py --resize device)
    runs = {"bicubic": FramePipeline(net, tf, h, w, decode=bicubic, out_height=ho, out_width=wo, **kw),
            "guided": FramePipeline(net, tf, h, w, out_height=H, out_width=W, upscale="guided", upscale_radius=RADIUS,
                                    upscale_eps=EPS, **kw)}
    sink = lambda i, a: None                                                # noqa: E731
    for p in runs.values():                 # warm-up: code objects, rings, workspaces of every stream
        p.run(frames[:16], sink)
    torch.cuda.synchronize()
    fps = {k: [] for k in runs}
    for _ in range(repeats):                # the variants alternate: drift of clocks and neighbours hits both alike
        for k, p in runs.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink)
            fps[k].append(n / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in fps.items()}
    return {"source": f"{W}x{H}", "working_size": f"{w}x{h}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
            "written_size": {"bicubic": f"{wo}x{ho} (the script's writer size for this clip)", "guided": f"{W}x{H}"},
            "host_bytes_out_per_frame": {"bicubic": 3 * wo * ho, "guided": 3 * W * H},
            "frames_per_s": {k: spread(v) for k, v in fps.items()},
            "ms_per_frame_at_median": {k: round(1e3 / v, 3) for k, v in med.items()},
            "guided_over_bicubic_at_median": round(med["guided"] / med["bicubic"], 4)}


def whole_frame_rate(n_frames=24):
    import torch
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from tools.video_e2e import natural_frame
    net, cw = make_net(), cWCT()
    H, W = SRC_HW
    distinct = [natural_frame(H, W, t, seed=7) for t in range(2)]
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    pipe = FramePipeline(net, lambda z, i: cw.transfer_with_stats(z, stats), H, W, depth=3, compute_streams=2)
    sink = lambda i, a: None                                                # noqa: E731
    pipe.run([distinct[i % 2] for i in range(6)], sink)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run([distinct[i % 2] for i in range(n_frames)], sink)
    return {"frame": f"{W}x{H}", "frames": n, "frames_per_s": round(n / (time.perf_counter() - t0), 2),
            "note": "one window, for context: the whole-frame stylisation the guided upscale stands in for"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "guided_upscale.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-whole-frame", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats is not None:
        return merge_stats(args.merge_stats, args.out)
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3 windows per variant")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided.py measures on the GPU; there is none here")
    if args.trace_run:
        return trace_run()
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec.update({"device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
                "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
                "hbm_streaming_bytes_per_s": HBM_STREAM_BYTES_PER_S, "kernels": kernel_times(args.launches, args.samples)})
    for k in rec["kernels"]:
        print(json.dumps(k), flush=True)
    if not args.skip_pipeline:
        rec["pipeline_2160p_source"] = pipeline_rates(args.frames, args.repeats)
        print(json.dumps(rec["pipeline_2160p_source"]), flush=True)
    if not args.skip_whole_frame:
        rec["whole_frame_2160p"] = whole_frame_rate()
        print(json.dumps(rec["whole_frame_2160p"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
