"""The optical flow measured (csrc/flow.hip, FramePipeline(temporal=True, flow="estimate"); DESIGN.md section 6, "Optical flow").

    python tools/bench_flow.py [--out profiles/flow_estimate.json] [--frames 200] [--repeats 3] [--samples 5] [--launches 10]

Workload: 1920x1080 frames.
(a) vst_flow_lk_u8 with the defaults (5 levels, 3 iterations, radius 3), with iters=1 and with levels=1; vst_flow_consistency and
    vst_temporal_l1_masked_u8 beside the floor of their bytes - what they read and write once, gathers counted as if they were
    streams - over the HBM rate measured for streaming kernels on this card (6.29 TB/s).  HIP events around `--launches`
    back-to-back calls after a warm-up, `--samples` such windows, median and min / max.
(b) FramePipeline on 1080p frames, host memory to host memory, plain cWCT, a sink that drops the frame: temporal=True with one
    shared device flow (the loop the tree had before the estimator), with flow="estimate", and with flow_mask=True on top;
    `--frames` frames per window, `--repeats` (at least 3) windows per variant, the variants ALTERNATING inside one process, in one
    session.
Clocks are not pinned and the card may be shared: read the spread next to every median.  No target is set for any number."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.bench_yuv import spread, time_launches  # noqa: E402

HBM_STREAM_BYTES_PER_S = 6.29e12       # measured float4 copy on this card (79 % of the 8.0 TB/s peak)
HW = (1080, 1920)
NOT_MEASURED = ["other frame sizes, radii and lambdas", "accuracy on real footage or against any published benchmark: the "
                "defaults are starting values checked on synthetic textures under smooth motion only",
                "the loop under --auto_seg, the windows or --preserve_luminance with the flags",
                "video_transfer.py end to end", "loss values on trained weights or real footage"]


def kernel_times(launches, samples):
    import ctypes as C
    import torch
    from vstnet_amd import _lib, flow, temporal
    from tools.video_e2e import natural_frame
    L, vp = _lib.lib(), C.c_void_p
    h, w = HW
    px = h * w
    a, b = (torch.from_numpy(natural_frame(h, w, t, seed=7)).cuda() for t in range(2))
    fwd, bwd = (torch.empty((2, h, w), dtype=torch.float32, device="cuda") for _ in range(2))
    valid = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    loss = torch.empty(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(flow.workspace_bytes(h, w, 5), dtype=torch.uint8, device="cuda")
    tws = torch.empty(temporal.workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = {k: vp(t.data_ptr()) for k, t in dict(a=a, b=b, fwd=fwd, bwd=bwd, valid=valid, loss=loss, ws=ws, tws=tws).items()}
    lk = lambda lv, it: (lambda: L.vst_flow_lk_u8(p["a"], p["b"], h, w, lv, it, 3, 1e-3, p["fwd"], p["ws"], st))  # noqa: E731
    _lib.check(L.vst_flow_lk_u8(p["b"], p["a"], h, w, 5, 3, 3, 1e-3, p["bwd"], p["ws"], st), "vst_flow_lk_u8")
    calls = [
        ("vst_flow_lk_u8", "levels 5, iters 3, radius 3", lk(5, 3), None),
        ("vst_flow_lk_u8", "levels 5, iters 1, radius 3", lk(5, 1), None),
        ("vst_flow_lk_u8", "levels 1, iters 3, radius 3", lk(1, 3), None),
        ("vst_flow_lk_u8", "levels 5, iters 3, radius 3 (again: the first line's twin)", lk(5, 3), None),
        ("vst_flow_consistency", "", lambda: L.vst_flow_consistency(p["fwd"], p["bwd"], h, w, p["valid"], st), (8 + 8 + 1) * px),
        ("vst_temporal_l1_masked_u8", "flow", lambda: L.vst_temporal_l1_masked_u8(p["a"], p["b"], p["fwd"], p["valid"], h, w,
                                                                                  p["loss"], None, p["tws"], st), (8 + 3 + 3 + 1) * px),
    ]
    out = []
    for name, form, call, nbytes in calls:
        _lib.check(call(), name)
        us = [time_launches(call, launches, warmup=3) * 1e6 for _ in range(samples)]
        rec = {"call": name, "form": form, "frame": f"{w}x{h}", "us": spread(us)}
        if nbytes is not None:
            floor = nbytes / HBM_STREAM_BYTES_PER_S * 1e6
            rec.update({"frame_bytes": nbytes, "frame_bytes_floor_us": round(floor, 2),
                        "time_over_floor_at_median": round(statistics.median(us) / floor, 2)})
        out.append(rec)
    torch.cuda.synchronize()
    out.append({"valid_share_of_the_pair": float(valid.float().mean()), "workspace_bytes": int(ws.numel()),
                "note": "two consecutive frames of tools/video_e2e.natural_frame: shows that the calls run on picture-like data"})
    return out


def pipeline_rates(n_frames, repeats):
    import numpy as np
    import torch
    from models.cWCT import cWCT
    from vstnet_amd import temporal
    from vstnet_amd.pipeline import FramePipeline
    from tools.bench_guided import make_net
    from tools.video_e2e import natural_frame
    net, cw = make_net(), cWCT()
    h, w = HW
    distinct = [natural_frame(h, w, t, seed=7) for t in range(4)]
    frames = [distinct[i % 4] for i in range(n_frames)]
    flow = temporal.fake_flow((h, w), np.random.default_rng(0), 8, 10, 100, 100)
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    kw = dict(depth=4, compute_streams=3, temporal=True)
    runs = {"shared_flow": (FramePipeline(net, tf, h, w, **kw), dict(flows=[None] + [flow] * (n_frames - 1))),
            "estimate": (FramePipeline(net, tf, h, w, flow="estimate", **kw), {}),
            "estimate_mask": (FramePipeline(net, tf, h, w, flow="estimate", flow_mask=True, **kw), {})}
    sink = lambda i, a: None                                                # noqa: E731
    for p, extra in runs.values():          # warm-up: code objects, rings, workspaces of every stream
        p.run(frames[:16], sink, **({k: v[:16] for k, v in extra.items()}))
    torch.cuda.synchronize()
    fps = {k: [] for k in runs}
    for _ in range(repeats):                # the variants alternate: drift of clocks and neighbours hits all alike
        for k, (p, extra) in runs.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink, **extra)
            fps[k].append(n / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in fps.items()}
    share = [v[2] for v in runs["estimate_mask"][0].temporal.values()]
    return {"frame": f"{w}x{h}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
            "frames_per_s": {k: spread(v) for k, v in fps.items()},
            "ms_per_frame_at_median": {k: round(1e3 / v, 3) for k, v in med.items()},
            "estimate_over_shared_flow_at_median": round(med["estimate"] / med["shared_flow"], 4),
            "estimate_mask_over_shared_flow_at_median": round(med["estimate_mask"] / med["shared_flow"], 4),
            "mean_valid_share": statistics.fmean(share),
            "note": "four frames in rotation: shows that the instrument runs; says nothing about a trained model or footage"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flow_estimate.json"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3 windows per variant")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow.py measures on the GPU; there is none here")
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec.update({"device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
                "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
                "hbm_streaming_bytes_per_s": HBM_STREAM_BYTES_PER_S, "not_measured": NOT_MEASURED,
                "kernels": kernel_times(args.launches, args.samples)})
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
