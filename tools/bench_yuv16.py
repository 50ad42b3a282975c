"""The high-bit-depth edge measured (csrc/yuv.hip vst_yuv16_to_rgb_f32 / vst_rgb_f32_to_yuv16, FramePipeline with a DeepYuvSpec
on both sides; DESIGN.md section 6, "High-bit-depth edge").

    python tools/bench_yuv16.py [--out profiles/yuv_deep.json] [--frames 300] [--repeats 3] [--samples 7] [--launches 200]

(a) the kernels at 1920x1080, yuv420p10le (4:2:0 left-sited, BT.709, limited range; the other layouts beside it): HIP events
    around `--launches` back-to-back calls of the C entry point (through ctypes, arguments made once) after a warm-up,
    `--samples` such windows, median and min / max.  bytes = what a launch must read and write once (12 per pixel of fp32 planes,
    2 per sample of the planes, 3 more per pixel with the u8 side output), so bytes/s is the algorithmic rate beside the
    streaming bound.  The same call on a 16x16 frame gives the floor of the method - the rate at which this host issues
    launches.
(b) FramePipeline at 1920x1080, host memory to host memory, plain cWCT, a sink that drops the frame: 10-bit 4:2:0 planes in and
    out against 8-bit 4:2:0 planes in and out - the loop of the commit before this edge - `--frames` frames per window,
    `--repeats` (at least 3) windows per variant, the variants ALTERNATING inside one process, in this one session.
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

from tools.bench_yuv import HBM_PEAK_BYTES_PER_S, spread, time_launches  # noqa: E402


def kernel_times(launches, samples, depth=10):
    import ctypes as C
    import torch
    from vstnet_amd import _lib
    from vstnet_amd.yuv import DeepYuvSpec
    L, vp = _lib.lib(), C.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    out = []
    for (H, W) in ((16, 16), (1080, 1920)):
        g = torch.Generator().manual_seed(H)
        rgb = torch.rand((1, 3, H, W), dtype=torch.float32, generator=g).cuda()
        for layout in ("420mpeg2", "420jpeg", "422", "444"):
            spec = DeepYuvSpec(layout, "bt709", "limited", depth)
            n = spec.frame_bytes(H, W) // 2
            flat = torch.randint(0, 1 << depth, (n,), dtype=torch.int16, generator=g).cuda().view(torch.uint8)
            dst_rgb, dst_u8, dst_flat = torch.empty_like(rgb), torch.empty((H, W, 3), dtype=torch.uint8, device="cuda"), torch.empty_like(flat)
            lay, mat, rng, _ = spec.codes
            ys, cs, _ = spec.plane_shapes(H, W)
            offs = (0, 2 * ys[0] * ys[1], 2 * (ys[0] * ys[1] + cs[0] * cs[1]))
            src = [vp(flat.data_ptr() + o) for o in offs]
            dst = [vp(dst_flat.data_ptr() + o) for o in offs]
            p_rgb, p_dst_rgb, p_u8 = vp(rgb.data_ptr()), vp(dst_rgb.data_ptr()), vp(dst_u8.data_ptr())
            calls = (("vst_yuv16_to_rgb_f32", 12 * H * W + 2 * n,
                      lambda: L.vst_yuv16_to_rgb_f32(src[0], src[1], src[2], H, W, depth, lay, mat, rng, p_dst_rgb, None, stream)),
                     ("vst_yuv16_to_rgb_f32 + u8", 15 * H * W + 2 * n,
                      lambda: L.vst_yuv16_to_rgb_f32(src[0], src[1], src[2], H, W, depth, lay, mat, rng, p_dst_rgb, p_u8, stream)),
                     ("vst_rgb_f32_to_yuv16", 12 * H * W + 2 * n,
                      lambda: L.vst_rgb_f32_to_yuv16(p_rgb, H, W, depth, lay, mat, rng, dst[0], dst[1], dst[2], stream)))
            for name, nbytes, fn in calls:
                _lib.check(fn(), name)
                us = [time_launches(fn, launches) * 1e6 for _ in range(samples)]
                med = statistics.median(us)
                out.append({"kernel": name, "frame": f"{W}x{H}" + (" (the method's floor)" if H == 16 else ""), "layout": layout,
                            "depth": depth, "us": spread(us), "bytes": nbytes, "gbytes_per_s_at_median": round(nbytes / med / 1e3, 1),
                            "streaming_bound_us": round(nbytes / HBM_PEAK_BYTES_PER_S * 1e6, 2)})
            if H == 16:
                break           # (one layout is enough for the floor)
    return out


def pipeline_rates(n_frames, repeats, H=1080, W=1920):
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict
    from vstnet_amd.yuv import DeepYuvSpec, YuvSpec, rgb_to_yuv16_host, rgb_to_yuv_host
    from tools.video_e2e import natural_frame
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234))
    net = net.to("cuda").eval()
    cw = cWCT()
    spec8, spec10 = YuvSpec("420mpeg2", "bt709", "limited"), DeepYuvSpec("420mpeg2", "bt709", "limited", 10)
    distinct = [natural_frame(H, W, t, seed=7) for t in range(4)]
    planes8 = [rgb_to_yuv_host(f, spec8) for f in distinct]
    planes10 = [rgb_to_yuv16_host(f / 255.0, spec10) for f in distinct]
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    kw = dict(depth=4, compute_streams=3)
    runs = {"yuv420p_in_yuv420p_out": (FramePipeline(net, tf, H, W, src_yuv=spec8, out_yuv=spec8, **kw),
                                       [planes8[i % 4] for i in range(n_frames)]),
            "yuv420p10le_in_yuv420p10le_out": (FramePipeline(net, tf, H, W, src_yuv=spec10, out_yuv=spec10, **kw),
                                               [planes10[i % 4] for i in range(n_frames)])}
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
           "host_bytes_per_frame_each_way": {"yuv420p_in_yuv420p_out": spec8.frame_bytes(H, W),
                                             "yuv420p10le_in_yuv420p10le_out": spec10.frame_bytes(H, W)},
           "frames_per_s": {k: spread(v) for k, v in fps.items()}}
    med = {k: statistics.median(v) for k, v in fps.items()}
    rec["ms_per_frame_at_median"] = {k: round(1e3 / v, 3) for k, v in med.items()}
    rec["deep_over_8_bit_at_median"] = round(med["yuv420p10le_in_yuv420p10le_out"] / med["yuv420p_in_yuv420p_out"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "yuv_deep.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3 windows per variant")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv16.py measures on the GPU; there is none here")
    rec = {"what": "the high-bit-depth edge: (a) kernel times at 10 bits per layout, (b) FramePipeline 10-bit 4:2:0 planes both "
                   "ways against 8-bit 4:2:0 planes both ways, alternating in one session",
           "device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
           "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
           "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "kernels": kernel_times(args.launches, args.samples)}
    for k in rec["kernels"]:
        print(json.dumps(k), flush=True)
    if not args.skip_pipeline:
        rec["pipeline_1080p"] = pipeline_rates(args.frames, args.repeats)
        print(json.dumps(rec["pipeline_1080p"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
