"""The temporal stabiliser measured (csrc/stabilise.hip, FramePipeline(temporal=True, stabilise=...); DESIGN.md section 6,
"Stabiliser").

    python tools/bench_stabilise.py [--out profiles/stabilise.json] [--frames 200] [--repeats 3] [--samples 5] [--launches 10]

Workload: 1920x1080 frames.
(a) vst_stabilise_u8 with the defaults, without and with a mask, beside the floor of its bytes - what it reads and writes once,
    the two gathers counted as if they were streams - over the HBM rate measured for streaming kernels on this card (6.29 TB/s).
    HIP events around `--launches` back-to-back calls after a warm-up, `--samples` such windows, median and min / max.
(b) FramePipeline on 1080p frames, host memory to host memory, plain cWCT, a sink that drops the frame, temporal=True with
    flow="estimate": without and with stabilise, and both again with flow_mask=True; `--frames` frames per window, `--repeats` (at
    least 3) windows per variant, the variants ALTERNATING inside one process, in one session.  The ratio is frames per second with
    the flag over frames per second without it, medians of the same session.
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
NOT_MEASURED = ["picture quality of the stabilised frames: real footage, trained weights",
                "good values of gain, sigma and limit: the defaults are starting values from a numpy prototype on constructed clips",
                "recursive blur over long clips", "other frame sizes", "the loop with given flows (--flow_dir, --synthetic_motion), "
                "the windows or --preserve_luminance with the flag", "video_transfer.py end to end"]


def kernel_times(launches, samples):
    import ctypes as C
    import torch
    from vstnet_amd import _lib, flow
    from tools.video_e2e import natural_frame
    L, vp = _lib.lib(), C.c_void_p
    h, w = HW
    px = h * w
    cur_in, prev_in, cur_out, prev_written = (torch.from_numpy(natural_frame(h, w, t, seed=7)).cuda() for t in (1, 0, 3, 2))
    fwd = flow.estimate_flow(cur_in, prev_in)
    valid = flow.consistency(fwd, flow.estimate_flow(prev_in, cur_in))
    written = torch.empty_like(cur_out)
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = {k: vp(t.data_ptr()) for k, t in dict(ci=cur_in, pi=prev_in, co=cur_out, pw=prev_written, fl=fwd, va=valid,
                                              wr=written).items()}
    call = lambda va: (lambda: L.vst_stabilise_u8(p["ci"], p["pi"], p["co"], p["pw"], p["fl"], va, h, w, 0.7, 8.0, 24.0,  # noqa: E731
                                                  p["wr"], st))
    out = []
    for form, fn, nbytes in (("gain 0.7, sigma 8, limit 24, no mask", call(None), (3 * 4 + 8 + 3) * px),
                             ("gain 0.7, sigma 8, limit 24, forward-backward mask", call(p["va"]), (3 * 4 + 8 + 1 + 3) * px)):
        _lib.check(fn(), "vst_stabilise_u8")
        us = [time_launches(fn, launches, warmup=3) * 1e6 for _ in range(samples)]
        floor = nbytes / HBM_STREAM_BYTES_PER_S * 1e6
        out.append({"call": "vst_stabilise_u8", "form": form, "frame": f"{w}x{h}", "us": spread(us), "frame_bytes": nbytes,
                    "frame_bytes_floor_us": round(floor, 2), "time_over_floor_at_median": round(statistics.median(us) / floor, 2)})
    torch.cuda.synchronize()
    out.append({"valid_share_of_the_pair": float(valid.float().mean()), "bytes_changed_share": float((written != cur_out).float().mean()),
                "note": "frames of tools/video_e2e.natural_frame: shows that the call runs on picture-like data"})
    return out


def pipeline_rates(n_frames, repeats):
    import torch
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from tools.bench_guided import make_net
    from tools.video_e2e import natural_frame
    net, cw = make_net(), cWCT()
    h, w = HW
    distinct = [natural_frame(h, w, t, seed=7) for t in range(4)]
    frames = [distinct[i % 4] for i in range(n_frames)]
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    kw = dict(depth=4, compute_streams=3, temporal=True, flow="estimate")
    runs = {"estimate": FramePipeline(net, tf, h, w, **kw),
            "estimate_stabilise": FramePipeline(net, tf, h, w, stabilise=True, **kw),
            "estimate_mask": FramePipeline(net, tf, h, w, flow_mask=True, **kw),
            "estimate_mask_stabilise": FramePipeline(net, tf, h, w, flow_mask=True, stabilise=True, **kw)}
    sink = lambda i, a: None                                                # noqa: E731
    for p in runs.values():                 # warm-up: code objects, rings, workspaces of every stream
        p.run(frames[:16], sink)
    torch.cuda.synchronize()
    fps = {k: [] for k in runs}
    for _ in range(repeats):                # the variants alternate: drift of clocks and neighbours hits all alike
        for k, p in runs.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink)
            fps[k].append(n / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in fps.items()}
    p = runs["estimate_stabilise"]
    raw = statistics.fmean(p.stabilised.values())
    out = statistics.fmean(v[0] for v in p.temporal.values())
    return {"frame": f"{w}x{h}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
            "frames_per_s": {k: spread(v) for k, v in fps.items()},
            "ms_per_frame_at_median": {k: round(1e3 / v, 3) for k, v in med.items()},
            "stabilise_over_plain_at_median": round(med["estimate_stabilise"] / med["estimate"], 4),
            "stabilise_over_plain_with_mask_at_median": round(med["estimate_mask_stabilise"] / med["estimate_mask"], 4),
            "mean_loss_raw": raw, "mean_loss_out": out,
            "note": "four frames in rotation under synthetic weights: shows that the loop runs and what it costs; the two losses "
                    "say nothing about a trained model or footage"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stabilise.json"))
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
        raise SystemExit("bench_stabilise.py measures on the GPU; there is none here")
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
