"""The style loss measured (csrc/vgg.hip, FramePipeline(style_loss=...); DESIGN.md section 6, "Style loss").

    python tools/bench_style_loss.py [--out profiles/style_loss.json] [--frames 60] [--repeats 3] [--samples 7] [--launches 5]

Workload: 1920x1080 frames, a 1280x720 style, the synthetic VGG weights (the arithmetic does not depend on the values).
(a) one StyleLoss call (loss_s alone, and with the content loss): HIP events around `--launches` back-to-back calls after a
    warm-up, `--samples` such windows, median and min / max.
(b) the same call's kernels one by one at the sizes the chain runs them at (the kernel-level calls of include/vstnet.h), timed
    the same way, and each one's share of their sum; beside each conv the bf16 MFMA work it issues (6 products x 2 M N K).
(c) conv1_2 (64 -> 64 at 1080p) once by the explicit route the implicit GEMM replaces: the reflect-padded map of one band of 60
    rows, vst_seg_im2col of it (the [band x 1920][576] column matrix) and vst_seg_gemm, scaled to the 18 bands of a frame, next
    to the implicit kernel on the whole frame, and the bytes the whole frame's column matrix would take.  (The band's result is
    checked against the implicit kernel's rows bit for bit.)
(d) FramePipeline on 1080p frames, host memory to host memory, plain cWCT, a sink that drops the frame, with and without
    style_loss, `--frames` frames per window, `--repeats` (at least 3) windows per variant, the variants ALTERNATING inside one
    process, in one session.
Clocks are not pinned and the card may be shared: read the spread next to every median.  No target is set for any number: the
call is new, there is nothing to compare a time against."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.bench_yuv import spread, time_launches  # noqa: E402

HW, STYLE_HW, BAND = (1080, 1920), (720, 1280), 60
# the chain of csrc/vgg.hip's vgg_features: (name, Cin, Cout, level) and what follows the conv
CHAIN = (("conv1_1", 4, 64, 0, "tap"), ("conv1_2", 64, 64, 0, "pool"), ("conv2_1", 64, 128, 1, "tap"), ("conv2_2", 128, 128, 1, "pool"),
         ("conv3_1", 128, 256, 2, "tap"), ("conv3_2", 256, 256, 2, None), ("conv3_3", 256, 256, 2, None),
         ("conv3_4", 256, 256, 2, "pool"), ("conv4_1", 256, 512, 3, "tap"))


def frames_u8(hw, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (hw[0], hw[1], 3), dtype=torch.uint8, generator=g).cuda()


def call_times(launches, samples):
    from vstnet_amd.vgg import StyleLoss, VGGEncoder, workspace_bytes
    enc = VGGEncoder("synthetic", "cuda:0")
    meter = StyleLoss(enc, frames_u8(STYLE_HW, 2))
    frame, content = frames_u8(HW, 3), frames_u8(HW, 4)
    out = {"workspace_bytes_per_slot": workspace_bytes(*HW)}
    for name, c in (("loss_s", None), ("loss_s_and_loss_c", content)):
        ms = [time_launches(lambda: meter(frame, c), launches, warmup=2) * 1e3 for _ in range(samples)]
        out[name + "_ms"] = spread(ms, 3)
    return out


def layer_times(launches, samples):
    import torch
    from vstnet_amd import vgg
    from vstnet_amd.vgg import level_sizes
    sizes = level_sizes(*HW)
    g = torch.Generator().manual_seed(5)
    rows, total = [], 0.0

    def timed(name, fn, extra=None):
        nonlocal total
        ms = [time_launches(fn, launches, warmup=2) * 1e3 for _ in range(samples)]
        rows.append(dict(kernel=name, ms=spread(ms, 3), **(extra or {})))
        total += statistics.median(ms)
    frame = frames_u8(HW, 3)
    w9, b3 = torch.randn(9, generator=g).cuda(), torch.randn(3, generator=g).cuda()
    timed("input_u8", lambda: vgg.input_map(frame, w9, b3))
    for name, cin, cout, level, after in CHAIN:
        h, w = sizes[level]
        x = torch.rand((h * w, cin), generator=g).cuda()
        wt = (torch.randn((cout, 9 * cin), generator=g) / (9 * cin) ** 0.5).cuda()
        b = torch.randn(cout, generator=g).cuda()
        flops = 6 * 2 * h * w * cout * 9 * cin
        timed(name, lambda: vgg.conv3x3_relu(x, wt, b, h, w), {"map": f"{w}x{h}", "cin": cin, "cout": cout, "mfma_flop": flops})
        rows[-1]["mfma_tflop_per_s_at_median"] = round(flops / (rows[-1]["ms"]["median"] * 1e-3) / 1e12, 1)
        y = torch.rand((h * w, cout), generator=g).cuda()
        del x
        if after == "tap":
            timed(f"mean_std relu{level + 1}_1", lambda: vgg.mean_std(y), {"map": f"{w}x{h}", "channels": cout})
        elif after == "pool":
            timed(f"maxpool after {name}", lambda: vgg.maxpool2(y, h, w), {"map": f"{w}x{h}", "channels": cout})
        del y
        torch.cuda.empty_cache()
    ra = torch.randn(vgg.RECORD_DOUBLES, dtype=torch.float64, generator=g).cuda()
    timed("style_loss", lambda: vgg.style_loss_of_records(ra, ra))
    h4, w4 = sizes[3]
    m = torch.rand((h4 * w4, 512), generator=g).cuda()
    timed("mse_f64 relu4_1", lambda: vgg.mse_f64(m, m))
    for r in rows:
        r["share_of_sum"] = round(r["ms"]["median"] / total, 4)
    return {"sum_of_medians_ms": round(total, 3), "kernels": rows,
            "note": "the kernel-level wrappers allocate their output per call; the chain itself allocates nothing"}


def explicit_conv1_2(launches, samples):
    import torch
    from vstnet_amd import vgg
    from vstnet_amd.segformer import ops
    h, w = HW
    g = torch.Generator().manual_seed(6)
    x = torch.rand((h * w, 64), generator=g).cuda()
    wt = (torch.randn((64, 576), generator=g) / 24.0).cuda()
    b = torch.randn(64, generator=g).cuda()
    implicit = [time_launches(lambda: vgg.conv3x3_relu(x, wt, b, h, w), launches, warmup=2) * 1e3 for _ in range(samples)]
    whole = vgg.conv3x3_relu(x, wt, b, h, w)
    # the band of rows 0 .. BAND-1 under the reflection: rows 1, 0 .. BAND, columns 1, 0 .. w-1, w-2
    m = x.view(h, w, 64)
    ry = torch.tensor([1] + list(range(BAND + 1)), device="cuda")
    rx = torch.tensor([1] + list(range(w)) + [w - 2], device="cuda")
    padded = m[ry][:, rx].reshape(-1, 64).contiguous()
    col = torch.empty((BAND * w, 576), dtype=torch.float32, device="cuda")
    out = torch.empty((BAND * w, 64), dtype=torch.float32, device="cuda")
    im2col = [time_launches(lambda: ops.im2col(padded, BAND + 2, w + 2, 3, 1, 0, out=col), launches, warmup=2) * 1e3
              for _ in range(samples)]
    gemm = [time_launches(lambda: ops.gemm(col, wt, b, out=out), launches, warmup=2) * 1e3 for _ in range(samples)]
    same = bool(torch.equal(torch.relu(out), whole[:BAND * w]))
    bands = h // BAND
    return {"frame": f"{w}x{h}", "band_rows": BAND, "bands_per_frame": bands, "implicit_whole_frame_ms": spread(implicit, 3),
            "explicit_band_im2col_ms": spread(im2col, 3), "explicit_band_gemm_ms": spread(gemm, 3),
            "explicit_whole_frame_ms_at_median": round(bands * (statistics.median(im2col) + statistics.median(gemm)), 3),
            "column_matrix_bytes_band": BAND * w * 576 * 4, "column_matrix_bytes_whole_frame": h * w * 576 * 4,
            "band_equals_implicit_bit_for_bit": same}


def pipeline_rates(n_frames, repeats):
    import torch
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline
    from vstnet_amd.vgg import StyleLoss, VGGEncoder
    from tools.bench_guided import make_net
    from tools.video_e2e import natural_frame
    net, cw = make_net(), cWCT()
    h, w = HW
    distinct = [natural_frame(h, w, t, seed=7) for t in range(4)]
    frames = [distinct[i % 4] for i in range(n_frames)]
    style = natural_frame(STYLE_HW[0], STYLE_HW[1], 3, seed=11)
    with torch.no_grad():
        stats = cw.style_stats(net.forward_u8(torch.from_numpy(style)[None].cuda()))
    tf = lambda z, i: cw.transfer_with_stats(z, stats)                      # noqa: E731
    meter = StyleLoss(VGGEncoder("synthetic", "cuda:0"), torch.from_numpy(style).cuda())
    kw = dict(depth=4, compute_streams=3)
    runs = {"plain": FramePipeline(net, tf, h, w, **kw), "style_loss": FramePipeline(net, tf, h, w, style_loss=meter, **kw)}
    sink = lambda i, a: None                                                # noqa: E731
    for p in runs.values():                 # warm-up: code objects, rings, workspaces of every slot
        p.run(frames[:12], sink)
    torch.cuda.synchronize()
    fps = {k: [] for k in runs}
    for _ in range(repeats):                # the variants alternate: drift of clocks and neighbours hits both alike
        for k, p in runs.items():
            t0 = time.perf_counter()
            n = p.run(frames, sink)
            fps[k].append(n / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in fps.items()}
    vals = [v[0] for v in runs["style_loss"].style.values()]
    return {"frame": f"{w}x{h}", "frames_per_window": n_frames, "depth": 4, "compute_streams": 3,
            "frames_per_s": {k: spread(v) for k, v in fps.items()},
            "ms_per_frame_at_median": {k: round(1e3 / v, 3) for k, v in med.items()},
            "style_loss_over_plain_at_median": round(med["style_loss"] / med["plain"], 4),
            "loss_s_on_synthetic_weights": {"mean": statistics.fmean(vals), "max": max(vals),
                                            "note": "shows that the instrument runs; says nothing about a trained model"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "style_loss.json"))
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3 windows per variant")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_style_loss.py measures on the GPU; there is none here")
    rec = {"device": torch.cuda.get_device_name(0), "launches_per_event_pair": args.launches,
           "clock_caveat": "clocks not pinned, card possibly shared: min / max stand next to every median",
           "frame": f"{HW[1]}x{HW[0]}", "style": f"{STYLE_HW[1]}x{STYLE_HW[0]}", "weights": "synthetic"}
    for key, fn in (("call", call_times), ("layers", layer_times), ("conv1_2_explicit_route", explicit_conv1_2)):
        rec[key] = fn(args.launches, args.samples)
        print(json.dumps({key: rec[key]}), flush=True)
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
