"""The temporal loss measured (csrc/temporal.hip, FramePipeline(temporal=True); DESIGN.md section 6, "Temporal loss").

    python tools/bench_temporal.py [--out profiles/temporal_loss.json] [--frames 300] [--repeats 3] [--samples 7] [--launches 50]

Workload: 1920x1080 frames under a fake flow of the reference's construction (100-pixel cells, a 100 x 100 blur).
(a) every entry point: HIP events around `--launches` back-to-back calls after a warm-up, `--samples` such windows, median and
    min / max.  Beside the time stands the floor of the call's bytes - what it reads and writes once, gathers counted as if they
    were streams - over the HBM rate measured for streaming kernels on this card (6.29 TB/s).
(b) FramePipeline on 1080p frames, host memory to host memory, plain cWCT, a sink that drops the frame, with and without
    temporal=True (one device flow for every frame, so the flag's uploads are not in the number), `--frames` frames per window,
    `--repeats` (at least 3) windows per variant, the variants ALTERNATING inside one process, in one session.  The loop without
    the flag is the loop the tree had before the flag existed.
Clocks are not pinned and the card may be shared: read the spread next to every median.  No target is set for either number."""
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
HW, CELL, KSIZE = (1080, 1920), 100, 100
NOT_MEASURED = ["other frame sizes", "the loop with one host flow per frame (a 16.6 MB upload each)", "the loop under --auto_seg, "
                "the windows or --preserve_luminance with the flag", "video_transfer.py end to end with .flo files read from disk",
                "loss values on trained weights or real footage: no window size or decay is recommended from these numbers"]


def kernel_times(launches, samples):
    import ctypes as C
    import numpy as np
    import torch
    from vstnet_amd import _lib, temporal
    L, vp = _lib.lib(), C.c_void_p
    h, w = HW
    px = h * w
    g = torch.Generator().manual_seed(1)
    au, bu = (torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(2))
    af, bf = (torch.rand((3, h, w), dtype=torch.float32, generator=g).cuda() for _ in range(2))
    noise = (0.001 * torch.randn((3, h, w), dtype=torch.float32, generator=g)).cuda()
    ou, of = torch.empty_like(au), torch.empty_like(af)
    grid_np, shifts = temporal.draw_fake_flow((h, w), np.random.default_rng(0), 8, 10, CELL)
    gh, gw = grid_np.shape[:2]
    grid = torch.from_numpy(grid_np).cuda()
    flow = torch.empty((2, h, w), dtype=torch.float32, device="cuda")
    fws = torch.empty(temporal.fake_flow_workspace_bytes(h, w, gh, gw, KSIZE), dtype=torch.uint8, device="cuda")
    loss = torch.empty(3, dtype=torch.float64, device="cuda")
    ws = torch.empty(temporal.workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = {k: vp(t.data_ptr()) for k, t in dict(au=au, bu=bu, af=af, bf=bf, noise=noise, ou=ou, of=of, grid=grid, flow=flow, fws=fws,
                                              loss=loss, ws=ws).items()}
    calls = [
        ("vst_fake_flow", "cell 100, ksize 100", lambda: L.vst_fake_flow(p["grid"], gh, gw, float(shifts[0]), float(shifts[1]), KSIZE,
                                                                         p["flow"], h, w, p["fws"], st), 8 * px),
        ("vst_warp_u8", "flow", lambda: L.vst_warp_u8(p["au"], p["flow"], None, p["ou"], h, w, st), (8 + 3 + 3) * px),
        ("vst_warp_u8", "flow, noise", lambda: L.vst_warp_u8(p["au"], p["flow"], p["noise"], p["ou"], h, w, st), (8 + 12 + 3 + 3) * px),
        ("vst_warp_f32", "flow", lambda: L.vst_warp_f32(p["af"], p["flow"], None, p["of"], h, w, st), (8 + 12 + 12) * px),
        ("vst_warp_f32", "flow, noise", lambda: L.vst_warp_f32(p["af"], p["flow"], p["noise"], p["of"], h, w, st), (8 + 36) * px),
        ("vst_temporal_l1_u8", "flow", lambda: L.vst_temporal_l1_u8(p["au"], p["bu"], p["flow"], h, w, p["loss"], None, p["ws"], st),
         (8 + 3 + 3) * px),
        ("vst_temporal_l1_u8", "no flow", lambda: L.vst_temporal_l1_u8(p["au"], p["bu"], None, h, w, p["loss"], None, p["ws"], st),
         (3 + 3) * px),
        ("vst_temporal_l1_u8", "flow, warped out", lambda: L.vst_temporal_l1_u8(p["au"], p["bu"], p["flow"], h, w, p["loss"], p["ou"],
                                                                                p["ws"], st), (8 + 3 + 3 + 3) * px),
        ("vst_temporal_l1_f32", "flow", lambda: L.vst_temporal_l1_f32(p["af"], p["bf"], p["flow"], h, w, p["loss"], None, p["ws"], st),
         (8 + 12 + 12) * px),
        ("vst_temporal_l1_f32", "no flow", lambda: L.vst_temporal_l1_f32(p["af"], p["bf"], None, h, w, p["loss"], None, p["ws"], st),
         (12 + 12) * px),
    ]
    out = []
    for name, form, call, nbytes in calls:
        _lib.check(call(), name)
        us = [time_launches(call, launches) * 1e6 for _ in range(samples)]
        floor = nbytes / HBM_STREAM_BYTES_PER_S * 1e6
        out.append({"call": name, "form": form, "frame": f"{w}x{h}", "us": spread(us), "frame_bytes": nbytes,
                    "frame_bytes_floor_us": round(floor, 2), "time_over_floor_at_median": round(statistics.median(us) / floor, 2)})
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
    flow = temporal.fake_flow((h, w), np.random.default_rng(0), 8, 10, CELL, KSIZE)
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(natural_frame(720, 1280, 3, seed=11))[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    kw = dict(depth=4, compute_streams=3)
    runs = {"plain": (FramePipeline(net, tf, h, w, **kw), {}),
            "temporal": (FramePipeline(net, tf, h, w, temporal=True, **kw), dict(flows=[None] + [flow] * (n_frames - 1)))}
    sink = lambda i, a: None                                                # noqa: E731
    for p, extra in runs.values():          # warm-up: code objects, rings, workspaces of every stream
        p.run(frames[:16], sink, **({k: v[:16] for k, v in extra.items()}))
    torch.cuda.synchronize()
    fps = {k: [] for k in runs}
    for _ in range(repeats):                # the variants alternate: drift of clocks and neighbours hits both alike
        for k, (p, extra) in runs.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink, **extra)
            fps[k].append(n / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in fps.items()}
    vals = list(runs["temporal"][0].temporal.values())
    return {"frame": f"{w}x{h}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
            "frames_per_s": {k: spread(v) for k, v in fps.items()},
            "ms_per_frame_at_median": {k: round(1e3 / v, 3) for k, v in med.items()},
            "temporal_over_plain_at_median": round(med["temporal"] / med["plain"], 4),
            "loss_on_synthetic_weights": {"mean_out": statistics.fmean(v[0] for v in vals), "mean_in": statistics.fmean(v[1] for v in vals),
                                          "note": "four unrelated frames in rotation under one flow: shows that the instrument "
                                                  "runs; says nothing about a trained model or about window sizes"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_loss.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3 windows per variant")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_temporal.py measures on the GPU; there is none here")
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
