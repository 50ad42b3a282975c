"""Luminance preservation at the uint8 frame edge measured (csrc/color.hip vst_lab_luminance_u8, vstnet_amd/pipeline.py
FramePipeline(preserve_luminance=True)).

    python tools/bench_luminance.py [--out profiles/luminance_edge.json] [--frames 120] [--samples 7] [--launches 100]

(a) the kernel: HIP events around `--launches` back-to-back launches after a warm-up, `--samples` such windows, median and
    min / max, at 1920x1080 and 1024x1024, both output forms; bytes = what the launch must read and write once (3 content + 12
    stylised + 3 or 12 out per pixel), so bytes/s is the algorithmic rate beside the streaming bound bytes / peak HBM bandwidth.
(b) FramePipeline at 1920x1080 (frames from host memory to host memory, plain cWCT, a sink that drops the frame) without and
    with preserve_luminance: frames/s of `--frames` frames after a warm-up run, `--samples` windows per variant, the variants
    ALTERNATING inside one process; the difference is the cost of the feature.
(c) the same loop with a `decode` hook that composes what the library offered before this edge: float decode, torch conversion
    of the uint8 frame (float, div, permute, contiguous), vst_lab_luminance, torch quantisation (mul, clamp, byte, permute,
    contiguous).
Clocks are not pinned and the card may be shared: read the spread next to every median.
"""
import argparse
import json
import os
import statistics
import sys
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
    import torch
    from vstnet_amd.color import luminance_transfer_u8
    out = []
    for (H, W) in ((1080, 1920), (1024, 1024)):
        g = torch.Generator().manual_seed(H)
        c = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, generator=g).cuda()
        s = (torch.rand((1, 3, H, W), generator=g) * 1.2 - 0.1).cuda()
        for to_float in (False, True):
            dst = torch.empty((1, 3, H, W), device="cuda") if to_float else torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda")
            us = [time_launches(lambda: luminance_transfer_u8(c, s, out=dst, to_float=to_float), launches) * 1e6
                  for _ in range(samples)]
            per_px = 3 + 12 + (12 if to_float else 3)
            nbytes = per_px * H * W
            med = statistics.median(us)
            out.append({"kernel": "vst_lab_luminance_u8_f32" if to_float else "vst_lab_luminance_u8", "frame": f"{W}x{H}",
                        "us": spread(us), "bytes_per_pixel": per_px, "bytes": nbytes,
                        "gbytes_per_s_at_median": round(nbytes / med / 1e3, 1),
                        "streaming_bound_us": round(nbytes / HBM_PEAK_BYTES_PER_S * 1e6, 2)})
    return out


def pipeline_rates(n_frames, samples, H=1080, W=1920):
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.color import luminance_transfer
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict
    from tools.video_e2e import natural_frame
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234))
    net = net.to("cuda").eval()
    cw = cWCT()
    distinct = [natural_frame(H, W, t, seed=7) for t in range(4)]
    frames = [distinct[i % 4] for i in range(n_frames)]
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731

    def composed(z, content_u8):           # the pieces the library had before the uint8 edge, chained on the frame's stream
        sty = net(z, forward=False)
        c = content_u8.float().div(255).permute(0, 3, 1, 2).contiguous()
        return luminance_transfer(c, sty).mul(255).clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous()
    pipes = {"without_flag": FramePipeline(net, tf, H, W, depth=4, compute_streams=3),
             "preserve_luminance": FramePipeline(net, tf, H, W, depth=4, compute_streams=3, preserve_luminance=True),
             "composed_hook": FramePipeline(net, tf, H, W, depth=4, compute_streams=3, preserve_luminance=True, decode=composed)}
    sink = lambda i, a: None                                                # noqa: E731
    fps = {k: [] for k in pipes}
    for k, p in pipes.items():              # warm-up: code objects, rings, workspaces of every stream
        p.run(frames[:24], sink)
    torch.cuda.synchronize()
    for _ in range(samples):                # the variants alternate: drift of clocks and neighbours hits all of them alike
        for k, p in pipes.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink)         # returns after the last frame was retired (its done event was synchronised)
            fps[k].append(n / (time.perf_counter() - t0))
    rec = {"frame": f"{W}x{H}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
           "frames_per_s": {k: spread(v) for k, v in fps.items()}}
    med = {k: statistics.median(v) for k, v in fps.items()}
    rec["ms_per_frame_at_median"] = {k: round(1e3 / v, 3) for k, v in med.items()}
    rec["cost_of_the_flag_ms_per_frame"] = round(1e3 / med["preserve_luminance"] - 1e3 / med["without_flag"], 3)
    rec["edge_over_composed_hook"] = round(med["preserve_luminance"] / med["composed_hook"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "luminance_edge.json"))
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_luminance.py measures on the GPU; there is none here")
    rec = {"what": "luminance preservation at the uint8 frame edge: (a) kernel times, (b) FramePipeline with and without the "
                   "flag, (c) against a decode hook composed of the float pieces",
           "device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
           "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
           "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "kernels": kernel_times(args.launches, args.samples)}
    for k in rec["kernels"]:
        print(json.dumps(k), flush=True)
    if not args.skip_pipeline:
        rec["pipeline_1080p"] = pipeline_rates(args.frames, args.samples)
        print(json.dumps(rec["pipeline_1080p"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
