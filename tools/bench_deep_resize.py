"""The deep resize measured (vst_yuv16_img_resize_f32, yuv.DeepImgResize, FramePipeline with src_deep_resize=True; DESIGN.md
section 6, "Deep resize").

    python tools/bench_deep_resize.py [--out profiles/deep_resize.json] [--frames 120] [--repeats 3] [--samples 7] [--launches 50]

(a) the resize of one 3840x2160 yuv420p10le frame (4:2:0 left-sited, BT.709, limited range) to 1280x720: HIP events around
    `--launches` back-to-back calls after a warm-up, `--samples` such windows per variant, the variants ALTERNATING window by
    window, median and min / max.  Variants: the shipped call (the fused first pass, then the vertical pass with the epilogue),
    with and without the u8 twin; and the UNFUSED COMPOSITION built from what the commit before this one had -
    vst_yuv16_to_rgb_f32 at the source size into a 100 MB fp32 frame, then vst_resize_f32's two plain float passes (its own
    weights and fp32 accumulation: the same traffic, not the same arithmetic).
(b) FramePipeline, host memory to host memory, plain cWCT at 1280x720, 10-bit 4:2:0 planes out, a sink that drops the frame:
    3840x2160 planes in through the deep resize, against conforming 1280x720 planes in - the loop of the commit before this one,
    the yardstick for what the resize (and the 25 MB upload) costs in the loop.  `--frames` frames per window, `--repeats` (at
    least 3) windows per variant, alternating inside one process, in this one session.
Clocks are not pinned and the card may be shared: read the spread next to every median.  One process, one GPU, no host thread
pool of its own; on a shared machine run it under a time limit of its own (`timeout -k 10 540 python
tools/bench_deep_resize.py`), chained with `&&` to whatever GPU step follows.
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

HS, WS, MAX_SIZE, H, W = 2160, 3840, 1280, 720, 1280


def kernel_times(launches, samples):
    import ctypes as C
    import torch
    from vstnet_amd import _lib
    from vstnet_amd.resize import _tables_on
    from vstnet_amd.yuv import DeepImgResize, DeepYuvSpec
    L, vp = _lib.lib(), C.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    spec = DeepYuvSpec("420mpeg2", "bt709", "limited", 10)
    n = spec.frame_bytes(HS, WS) // 2
    flat = torch.randint(0, 1 << 10, (n,), dtype=torch.int16, generator=torch.Generator().manual_seed(1)).cuda().view(torch.uint8)
    rs = DeepImgResize((HS, WS), spec, MAX_SIZE, 4, "cuda")
    assert rs.size_wh == (W, H)
    out = torch.empty((1, 3, H, W), dtype=torch.float32, device="cuda")
    out_u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    # the composition's buffers: the source-size fp32 frame, vst_resize_f32's pass buffer and tables
    rgb = torch.empty((1, 3, HS, WS), dtype=torch.float32, device="cuda")
    tmp = torch.empty(3 * HS * W, dtype=torch.float32, device="cuda")
    tables = _tables_on("f32", rgb.device, [(WS, W), (HS, H)])
    lay, mat, rng, depth = spec.codes
    ys, cs, _ = spec.plane_shapes(HS, WS)
    src = [vp(flat.data_ptr() + o) for o in (0, 2 * ys[0] * ys[1], 2 * (ys[0] * ys[1] + cs[0] * cs[1]))]
    p_rgb, p_tmp, p_tab, p_out, p_u8 = (vp(t.data_ptr()) for t in (rgb, tmp, tables, out, out_u8))

    def unfused():
        rc = L.vst_yuv16_to_rgb_f32(src[0], src[1], src[2], HS, WS, depth, lay, mat, rng, p_rgb, None, stream)
        return rc or L.vst_resize_f32(p_rgb, 1, HS, WS, p_out, H, W, p_tab, p_tmp, stream)

    # bytes a variant must move once: planes in, output out, and every intermediate written and read again
    planes, frame = 2 * n, 12 * H * W
    p_tab64, p_work = vp(rs.tables.data_ptr()), vp(rs.work.data_ptr())

    def fused(twin):
        return L.vst_yuv16_img_resize_f32(src[0], src[1], src[2], HS, WS, depth, lay, mat, rng, len(rs.steps), rs._steps, p_tab64,
                                          p_work, p_out, twin, stream)
    variants = {"fused": (lambda: fused(None), planes + 2 * 12 * HS * W + frame),
                "fused + u8 twin": (lambda: fused(p_u8), planes + 2 * 12 * HS * W + frame + 3 * H * W),
                "unfused composition (the parent's calls)": (unfused, planes + 2 * 12 * HS * WS + 2 * 12 * HS * W + frame)}
    for name, (fn, _) in variants.items():
        _lib.check(fn(), name)
    us = {k: [] for k in variants}
    for _ in range(samples):                # the variants alternate window by window
        for name, (fn, _) in variants.items():
            us[name].append(time_launches(fn, launches) * 1e6)
    recs = []
    for name, (_, nbytes) in variants.items():
        med = statistics.median(us[name])
        recs.append({"variant": name, "frame": f"{WS}x{HS} -> {W}x{H}", "pix_fmt": "yuv420p10le", "us": spread(us[name]),
                     "bytes": nbytes, "gbytes_per_s_at_median": round(nbytes / med / 1e3, 1),
                     "streaming_bound_us": round(nbytes / HBM_PEAK_BYTES_PER_S * 1e6, 2)})
    f, u = us["fused"], us["unfused composition (the parent's calls)"]
    verdict = {"fused_over_unfused_at_median": round(statistics.median(f) / statistics.median(u), 4),
               "fused_faster_outside_the_spread": max(f) < min(u)}
    return recs, verdict


def pipeline_rates(n_frames, repeats):
    import torch
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.synth import synthetic_state_dict
    from vstnet_amd.yuv import DeepYuvSpec, rgb_to_yuv16_host
    from tools.video_e2e import natural_frame
    net = RevResNet(hidden_dim=16, sp_steps=2)
    net.load_state_dict(synthetic_state_dict(1234))
    net = net.to("cuda").eval()
    cw = cWCT()
    spec = DeepYuvSpec("420mpeg2", "bt709", "limited", 10)
    big = [rgb_to_yuv16_host(natural_frame(HS, WS, t, seed=7) / 255.0, spec) for t in range(2)]
    small = [rgb_to_yuv16_host(natural_frame(H, W, t, seed=7) / 255.0, spec) for t in range(2)]
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    kw = dict(depth=4, compute_streams=3, src_yuv=spec, out_yuv=spec)
    runs = {"conforming_1280x720_in": (FramePipeline(net, tf, H, W, **kw), [small[i % 2] for i in range(n_frames)]),
            "3840x2160_in_deep_resize": (FramePipeline(net, tf, H, W, src_height=HS, src_width=WS, max_size=MAX_SIZE,
                                                       src_deep_resize=True, **kw), [big[i % 2] for i in range(n_frames)])}
    sink = lambda i, a: None                                                # noqa: E731
    for p, frames in runs.values():         # warm-up: code objects, rings, workspaces of every stream
        p.run(frames[:16], sink)
    torch.cuda.synchronize()
    fps = {k: [] for k in runs}
    for _ in range(repeats):                # the variants alternate: drift of clocks and neighbours hits both alike
        for k, (p, frames) in runs.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink)
            fps[k].append(n / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in fps.items()}
    return {"stylised_frame": f"{W}x{H}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
            "host_bytes_per_frame_in": {"conforming_1280x720_in": spec.frame_bytes(H, W),
                                        "3840x2160_in_deep_resize": spec.frame_bytes(HS, WS)},
            "frames_per_s": {k: spread(v) for k, v in fps.items()},
            "ms_per_frame_at_median": {k: round(1e3 / v, 3) for k, v in med.items()},
            "resize_over_conforming_at_median": round(med["3840x2160_in_deep_resize"] / med["conforming_1280x720_in"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deep_resize.json"))
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3 windows per variant")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_deep_resize.py measures on the GPU; there is none here")
    kernels, verdict = kernel_times(args.launches, args.samples)
    rec = {"what": "the deep resize: (a) 3840x2160 yuv420p10le -> 1280x720, the fused call against the unfused composition of the "
                   "parent's calls, alternating; (b) FramePipeline with the resize against conforming 1280x720 frames in, alternating",
           "device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
           "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
           "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "resize_2160p_to_720p": kernels, "verdict": verdict}
    for k in kernels + [verdict]:
        print(json.dumps(k), flush=True)
    if not args.skip_pipeline:
        rec["pipeline"] = pipeline_rates(args.frames, args.repeats)
        print(json.dumps(rec["pipeline"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
