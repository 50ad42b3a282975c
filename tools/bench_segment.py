#!/usr/bin/env python
"""On-device segmentation, measured: ms per frame of SegFormer-B4 (synthetic weights) at 1280x720, and the frame rate of the
video loop (FramePipeline, synthetic photorealistic weights, uint8 frames in and out) with the segmenter making every frame's
label map, next to the same loop fed one uploaded map per frame.  Prints one JSON line.

    python tools/bench_segment.py [--variant b4] [--height 720] [--width 1280] [--frames 24] [--warmup 3] [--flops]
                                  [--work_size S] [--argmax_ab] [--seg_window W]

--work_size S segments at the working resolution of --seg_size S (segmenter and video loop; the uploaded maps of the loop it is
compared with are made the same way).  --argmax_ab times only the last step, logits -> labels, with the per-pixel and with the
tiled sampler on the same logits (those of the working frame), checks that the two maps are equal, and prints that alone.
--seg_window W (2..8) adds the video loop with a temporal logit window of W frames (FramePipeline(seg_window=W), uniform
weights) and the time of the mixing kernel alone (vst_seg_mix_logits over W tensors of the loop's logit size, timed like the
segmenter) to the line.  (Back-to-back launches on the same W + 1 tensors: the Infinity Cache may hold them, so the kernel's
time in the loop, between other frames' kernels, is at least this.)
--flops prints the per-stage GEMM / attention FLOPs and activation bytes of the shape (host only, no GPU needed).
Timing: HIP events around `frames` back-to-back runs on one stream after `warmup` runs; the median of 5 such batches."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS, HEADS, SR = (64, 128, 320, 512), (1, 2, 5, 8), (8, 4, 2, 1)


def stage_table(depths, h, w, e=768):
    """[(name, GFLOP, MB of activations written)] per stage and for the head; a multiply-add counts as 2 FLOP."""
    hp, wp = (h + 3) // 4 * 4, (w + 3) // 4 * 4
    gh, gw = hp // 4, wp // 4
    rows, grids, cin = [], [], 3
    for s, c in enumerate(DIMS):
        if s:
            gh, gw = (gh - 1) // 2 + 1, (gw - 1) // 2 + 1
        grids.append((gh, gw))
        t, tk = gh * gw, (gh // SR[s]) * (gw // SR[s])
        k = 49 * 3 if s == 0 else 9 * cin
        f = 2 * t * c * k
        b = 4 * t * (k + c)
        per = 2 * t * c * c * 2                      # q, proj
        per += (2 * tk * c * SR[s] ** 2 * c if SR[s] > 1 else 0) + 2 * tk * 2 * c * c      # sr, kv
        per += 4 * t * tk * c                        # scores + weighted sum over all heads
        per += 2 * t * c * 4 * c * 2 + 2 * t * 4 * c * 9     # fc1, fc2, depthwise
        bper = 4 * t * (c * 5 + 4 * c * 2) + 4 * tk * (SR[s] ** 2 * c + 3 * c)
        rows.append((f"stage {s + 1} ({gh}x{gw}, C={c}, {depths[s]} blocks, {tk} keys)", (f + depths[s] * per) / 1e9,
                     (b + depths[s] * bper) / 1e6))
        cin = c
    t1 = grids[0][0] * grids[0][1]
    head = sum(2 * g[0] * g[1] * e * c for g, c in zip(grids, DIMS)) + 2 * t1 * e * 150
    unfolded = sum(2 * g[0] * g[1] * e * c for g, c in zip(grids, DIMS)) + 2 * t1 * 4 * e * e + 2 * t1 * e * 150
    rows.append((f"decode head, folded (unfolded: {unfolded / 1e9:.1f} GFLOP)", head / 1e9,
                 4 * (sum(g[0] * g[1] for g in grids) * e + t1 * 150) / 1e6))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="b4")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flops", action="store_true")
    ap.add_argument("--no_video", action="store_true")
    ap.add_argument("--work_size", type=int, default=None)
    ap.add_argument("--argmax_ab", action="store_true")
    ap.add_argument("--seg_window", type=int, default=1)
    a = ap.parse_args()
    from vstnet_amd.synth import SEG_DEPTHS, synthetic_scene_u8, synthetic_segformer_state_dict, synthetic_state_dict
    depths = SEG_DEPTHS[a.variant]
    if a.flops:
        total = 0.0
        for name, gf, mb in stage_table(depths, a.height, a.width):
            total += gf
            print(f"{name}: {gf:.1f} GFLOP, {mb:.0f} MB")
        print(f"total {total:.1f} GFLOP (x6 MFMA products for the GEMM part: three-way bf16 split)")
        return
    import torch
    from vstnet_amd.segformer import SegFormer
    H, W = a.height, a.width
    seg = SegFormer(a.variant, embedding_dim=256 if a.variant == "b1" else 768)
    seg.load_state_dict(synthetic_segformer_state_dict(4321, depths, seg.embedding_dim))
    frame = torch.from_numpy(synthetic_scene_u8(H, W, 0)).cuda()
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    hw, ww = seg.work_hw(H, W, a.work_size)
    work = torch.empty((hw, ww, 3), dtype=torch.uint8, device="cuda")
    if a.argmax_ab:
        import ctypes as C
        from vstnet_amd import _lib
        from vstnet_amd.resize import resize_u8
        lg = seg.logits(resize_u8(frame, (ww, hw)) if (hw, ww) != (H, W) else frame)[0]
        hq, wq = int(lg.shape[1]), int(lg.shape[2])
        lg = lg.permute(1, 2, 0).contiguous()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        res = {"height": H, "width": W, "work_height": hw, "work_width": ww, "logit_grid": [hq, wq], "scale": round(H / hq, 2)}
        maps = []
        for kernel, name in ((0, "per_pixel_ms"), (1, "tiled_ms")):
            o = torch.empty((H, W), dtype=torch.uint8, device="cuda")
            run = lambda: _lib.check(_lib.lib().vst_seg_labels_from_logits(       # noqa: E731
                C.c_void_p(lg.data_ptr()), hq, wq, H, W, kernel, C.c_void_p(o.data_ptr()), st), "vst_seg_labels_from_logits")
            for _ in range(a.warmup):
                run()
            batches = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.frames):
                    run()
                e1.record()
                e1.synchronize()
                batches.append(e0.elapsed_time(e1) / a.frames)
            res[name] = float(np.median(batches))
            maps.append(o)
        res["equal"] = bool(torch.equal(maps[0], maps[1]))
        print(json.dumps(res))
        return
    kw_seg = {} if a.work_size is None else {"work_size": a.work_size, "work": work}
    for _ in range(a.warmup):
        seg.segment_u8(frame, out=out, **kw_seg)
    torch.cuda.synchronize()
    batches = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.frames):
            seg.segment_u8(frame, out=out, **kw_seg)
        e1.record()
        e1.synchronize()
        batches.append(e0.elapsed_time(e1) / a.frames)
    res = {"variant": a.variant, "height": H, "width": W, "work_size": a.work_size, "work_height": hw, "work_width": ww,
           "segment_ms_per_frame": float(np.median(batches)),
           "segment_ms_batches": [round(b, 3) for b in batches], "labels_in_frame": int(torch.unique(out).numel())}
    if not a.no_video:
        from models.RevResNet import RevResNet
        from models.cWCT import cWCT
        from vstnet_amd.pipeline import FramePipeline
        net = RevResNet(hidden_dim=16, sp_steps=2)
        net.load_state_dict(synthetic_state_dict(1234, 16, 2))
        net = net.cuda().eval()
        cw = cWCT()
        frames = [synthetic_scene_u8(H, W, i) for i in range(4)]
        style = torch.from_numpy(synthetic_scene_u8(H, W, 50)).cuda()
        sty = seg.segment_u8(style, work_size=a.work_size).cpu().numpy()
        maps = [seg.segment_u8(torch.from_numpy(f).cuda(), work_size=a.work_size).cpu().numpy() for f in frames]
        with torch.no_grad():
            binding = cw.bind_style_labels(net.forward_u8(style[None]), sty)

        def plan(ms, cap):
            buf = ms.state.get("buffers")
            if buf is None:
                buf = ms.state["buffers"] = cw.frame_buffers(H, W, 32, "cuda")
            return cw.plan_frame(ms.mask, binding, max_slots=cap, buffers=buf, flags=ms.flags)
        tr = lambda z, i, ms: cw.transfer_with_plan(z, None, plan(ms, 8))          # noqa: E731
        rd = lambda z, i, ms: cw.transfer_with_plan(z, None, plan(ms, 32))         # noqa: E731
        n = a.frames
        configs = [("video_fps_uploaded_maps", {}, True), ("video_fps_auto_seg", {"segmenter": seg, "seg_work_size": a.work_size}, False)]
        if a.seg_window > 1:
            from vstnet_amd.segformer import window_weights
            configs.append(("video_fps_auto_seg_window", {"segmenter": seg, "seg_work_size": a.work_size, "seg_window": a.seg_window},
                            False))
            hq, wq = seg.logit_grid(hw, ww)
            lgs = [torch.randn((hq * wq, 150), device="cuda") for _ in range(a.seg_window)]
            mixed, wts = torch.empty_like(lgs[0]), window_weights(a.seg_window)
            for _ in range(a.warmup):
                seg.mix_logits(lgs, wts, mixed)
            batches = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.frames):
                    seg.mix_logits(lgs, wts, mixed)
                e1.record()
                e1.synchronize()
                batches.append(e0.elapsed_time(e1) / a.frames)
            res.update(seg_window=a.seg_window, logit_grid=[hq, wq], mix_ms=float(np.median(batches)),
                       mix_mb_moved=round((a.seg_window + 1) * hq * wq * 150 * 4 / 1e6, 1))
        for key, kw, masks in configs:
            pipe = FramePipeline(net, tr, H, W, redo=rd, compute_streams=3, **kw)
            src = lambda: (frames[i % 4] for i in range(n))                        # noqa: E731
            mk = lambda: (maps[i % 4] for i in range(n)) if masks else None        # noqa: E731
            pipe.run(src(), lambda i, f: None, masks=mk())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.run(src(), lambda i, f: None, masks=mk())
            torch.cuda.synchronize()
            res[key] = n / (time.perf_counter() - t0)
            res[key.replace("fps", "redo")] = pipe.redo_count
    print(json.dumps(res))


if __name__ == "__main__":
    main()
