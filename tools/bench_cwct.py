"""Time the cWCT statistics / apply entry points alone (unmasked vs the single-pass label-slot forms).

--any-width: the width-generic entry points (vst_cwct_stats_n / factor_n / apply_n, csrc/cwct_any.hip) at L = 2^20 for
N in {8, 24, 48, 96, 256}, and at N = 32 and 128 next to the tuned kernels (exact fp32 apply)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vstnet_amd import _lib                      # noqa: E402
from vstnet_amd.cwct import cWCT                 # noqa: E402
from vstnet_amd.synth import synthetic_mask      # noqa: E402


def timeit(fn, iters=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def any_width(L=1 << 20):
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    p = lambda t: C.c_void_p(t.data_ptr())                                         # noqa: E731
    null, st = C.c_void_p(0), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"L = {L}: times in us; GB/s = bytes moved (stats: N L 4 read; apply: 2 N L 4) / time")
    for N in (8, 24, 32, 48, 96, 128, 256):
        g = torch.Generator(device=dev).manual_seed(N)
        x = torch.randn(N, L, device=dev, generator=g) + 3.0
        y = torch.empty_like(x)
        stats = torch.empty(1 + N + N * N, dtype=torch.float64, device=dev)
        nws = lib.vst_cwct_stats_n_workspace_bytes(N, L)
        ws = torch.empty(max(nws, 1 << 20), dtype=torch.uint8, device=dev)
        t_s = timeit(lambda: _lib.check(lib.vst_cwct_stats_n(p(x), N, L, null, 0, p(stats), p(ws), ws.numel(), st), "stats_n"))
        fws = torch.empty(lib.vst_cwct_factor_n_workspace_bytes(N), dtype=torch.uint8, device=dev)
        aff = torch.empty(N * N + N, dtype=torch.float32, device=dev)
        info = torch.zeros(3, dtype=torch.int32, device=dev)
        styles, al = (C.c_void_p * 1)(stats.data_ptr()), (C.c_float * 1)(1.0)
        t_f = timeit(lambda: _lib.check(lib.vst_cwct_factor_n(p(stats), styles, al, 1, 0.0, 2e-5, N, p(aff), p(info), p(fws),
                                                              fws.numel(), st), "factor_n"), iters=5)
        t_a = timeit(lambda: _lib.check(lib.vst_cwct_apply_n(p(x), p(y), N, L, p(aff), null, 0, st), "apply_n"))
        gb = N * L * 4 / 1e3
        line = (f"N={N:3d}  _n: stats {t_s:8.1f} ({gb / t_s:6.0f} GB/s)  factor {t_f:8.1f}  apply {t_a:8.1f} "
                f"({2 * gb / t_a:6.0f} GB/s)")
        if N in (32, 128):
            tws = torch.empty(lib.vst_cwct_stats_workspace_bytes(N, L), dtype=torch.uint8, device=dev)
            t_ts = timeit(lambda: _lib.check(lib.vst_cwct_stats(p(x), N, L, null, 0, p(stats), p(tws), st), "stats"))
            t_ta = timeit(lambda: _lib.check(lib.vst_cwct_apply_prec(p(x), p(y), N, L, p(aff), null, 0, _lib.PREC_FP32, st),
                                             "apply_prec"))
            line += f"   | tuned: stats {t_ts:8.1f} ({gb / t_ts:6.0f} GB/s)  apply fp32 {t_ta:8.1f} ({2 * gb / t_ta:6.0f} GB/s)"
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--labels", type=int, default=5)
    ap.add_argument("--any-width", action="store_true", help="time the width-generic _n entry points instead")
    args = ap.parse_args()
    if args.any_width:
        return any_width()
    H, W, N = args.height, args.width, args.channels
    dev = torch.device("cuda", 0)
    cw = cWCT()
    z = torch.randn(1, N, H, W, device=dev)
    zs = torch.randn(1, N, H, W, device=dev) * 0.5 + 0.1
    x2 = z.reshape(N, -1)
    print(f"unmasked stats {timeit(lambda: cw.stats(x2)):8.1f} us   apply {timeit(lambda: cw.apply(x2, cw.factor(cw.stats(x2), [cw.stats(zs.reshape(N, -1))], [1.0], 0.0, N))):8.1f} us (incl. stats x2 + factor)")
    for kind in ("bands", "noise"):
        cm = synthetic_mask(H, W, args.labels, seed=3, kind=kind)[None]
        sm = synthetic_mask(H, W, args.labels, seed=4, speck=False, kind=kind)[None]
        plan = cw.learn_slots(cw.plan_masks(cm, sm, z.shape, zs.shape, dev))
        t_stats = timeit(lambda: cw._stats_labels(x2, plan.cm[0], plan.tables[0], plan.max_slots))
        bound = cw.bind_style(plan, zs)
        t_all = timeit(lambda: cw.transfer_with_plan(z, None, bound))
        print(f"{kind:6s} labels={args.labels}: stats_labels {t_stats:8.1f} us   transfer_with_plan {t_all:8.1f} us")


if __name__ == "__main__":
    main()
