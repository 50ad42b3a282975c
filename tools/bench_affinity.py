"""The affinity loss measured (csrc/matting.hip, FramePipeline(affinity=True); DESIGN.md section 6, "Affinity loss").

    python tools/bench_affinity.py [--out profiles/matting_loss.json] [--frames 300] [--repeats 3] [--samples 7] [--launches 50]

Workload: 1920x1080 frames, radius 1, eps 1e-7 (the reference's defaults).
(a) the two entry points, with and without the gradient: HIP events around `--launches` back-to-back calls after a warm-up,
    `--samples` such windows, median and min / max.  Beside the time stands the floor of the call's bytes - 3 B of guide and 12 B
    (float form; 3 B for the uint8 form) of x read per pixel, 12 B written when the gradient is on - over the HBM rate measured for
    streaming kernels on this card (6.29 TB/s).  The kernel is fp64 arithmetic out of LDS: the floor is where it cannot get to,
    not a target.
(b) FramePipeline on 1080p frames, host memory to host memory, plain cWCT, a sink that drops the frame, with and without
    affinity=True, `--frames` frames per window, `--repeats` (at least 3) windows per variant, the variants ALTERNATING inside
    one process, in one session.
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
HW, RADIUS, EPS = (1080, 1920), 1, 1e-7


def kernel_times(launches, samples):
    import ctypes as C
    import torch
    from vstnet_amd import _lib, matting
    L, vp = _lib.lib(), C.c_void_p
    h, w = HW
    g = torch.Generator().manual_seed(1)
    guide = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda()
    xf = torch.rand((3, h, w), dtype=torch.float32, generator=g).cuda()
    xu = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda()
    loss = torch.empty(3, dtype=torch.float64, device="cuda")
    grad = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    ws = torch.empty(matting.workspace_bytes(h, w, RADIUS), dtype=torch.uint8, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = {k: vp(t.data_ptr()) for k, t in dict(guide=guide, xf=xf, xu=xu, loss=loss, grad=grad, ws=ws).items()}
    out = []
    for name, fn, x, xbytes in (("vst_matting_loss_f32", L.vst_matting_loss_f32, p["xf"], 12),
                                ("vst_matting_loss_u8", L.vst_matting_loss_u8, p["xu"], 3)):
        for with_grad in (False, True):
            call = lambda: fn(p["guide"], x, h, w, RADIUS, EPS, p["loss"], p["grad"] if with_grad else None, p["ws"], st)  # noqa: E731
            _lib.check(call(), name)
            us = [time_launches(call, launches) * 1e6 for _ in range(samples)]
            nbytes = (3 + xbytes + (12 if with_grad else 0)) * h * w
            floor = nbytes / HBM_STREAM_BYTES_PER_S * 1e6
            out.append({"call": name, "gradient": with_grad, "frame": f"{w}x{h}", "radius": RADIUS, "us": spread(us),
                        "frame_bytes": nbytes, "frame_bytes_floor_us": round(floor, 2),
                        "time_over_floor_at_median": round(statistics.median(us) / floor, 2)})
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
    kw = dict(depth=4, compute_streams=3)
    runs = {"plain": FramePipeline(net, tf, h, w, **kw),
            "affinity": FramePipeline(net, tf, h, w, affinity=True, affinity_radius=RADIUS, affinity_eps=EPS, **kw)}
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
    vals = [float(v.sum()) for v in runs["affinity"].affinity.values()]
    return {"frame": f"{w}x{h}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
            "frames_per_s": {k: spread(v) for k, v in fps.items()},
            "ms_per_frame_at_median": {k: round(1e3 / v, 3) for k, v in med.items()},
            "affinity_over_plain_at_median": round(med["affinity"] / med["plain"], 4),
            "loss_on_synthetic_weights": {"mean": statistics.fmean(vals), "max": max(vals),
                                          "note": "shows that the instrument runs; says nothing about a trained model"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "matting_loss.json"))
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
        raise SystemExit("bench_affinity.py measures on the GPU; there is none here")
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec.update({"device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
                "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
                "hbm_streaming_bytes_per_s": HBM_STREAM_BYTES_PER_S, "kernels": kernel_times(args.launches, args.samples)})
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
