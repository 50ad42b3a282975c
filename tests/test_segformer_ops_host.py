"""The per-kernel SegFormer tests, host side (tests/segformer_ops_ref.py; the GPU side is tests/test_gpu_segformer_ops.py).

At every case of the GPU file the fp32 restatement of the device arithmetic sits at or under FACTOR / 2, and every mutant of it
exceeds 1.25 x FACTOR at one case at least: the bounds the device is held to have room for another summation order and none for
a lost product, a skipped rescale or a wrong divisor.  The fp64 op references are composed into the network's blocks and compared
with tests/segformer_ref.py, which pins the layout conventions.  Every test prints its ratios (-s)."""
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import segformer_ops_ref as O                                          # noqa: E402
import segformer_ref as R                                              # noqa: E402

NAMES = ["vst_seg_gemm", "vst_seg_layernorm", "vst_seg_attention", "vst_seg_dwconv_gelu", "vst_seg_im2col", "vst_seg_gather_rgb",
         "vst_seg_head_sum"]
TEETH = 1.25


def d(*ts):
    return [None if t is None else t.double() for t in ts]


def built_library():
    """the library, built first on a tree that was never built (as tests/test_host.py does): these tests always assert"""
    from vstnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def check_teeth(op, worst, mutants):
    """worst = {mutant: (ratio, case)}: every mutant misses the bound somewhere"""
    for m in mutants:
        print(f"{op} mutant '{m}': {worst[m][0]:.3g} x at {worst[m][1]} (needs > {TEETH * O.FACTOR[op]})")
        assert worst[m][0] > TEETH * O.FACTOR[op], (m, worst[m])


def test_gemm_restatement_and_mutants():
    cases = [(s, b, r) for s in O.GEMM_SHAPES for b in (False, True) for r in (False, True)] + [(s, False, False) for s in O.GEMM_SPECIAL]
    worst = {m: (0.0, None) for m in O.GEMM_MUTANTS}
    for shape, hb, hr in cases:
        if isinstance(shape, str):
            (a, w), bias, res = O.gemm_special(shape), None, None
        else:
            a, w, bias, res = O.gemm_inputs(*shape)
            bias, res = (bias if hb else None), (res if hr else None)
        want = O.gemm(*d(a, w, bias, res))
        e32 = O.gemm_err(O.fp32(O.gemm, a, w, bias, res), want, a, w, bias, res)
        r = O.ratio("gemm", O.gemm_err(O.gemm_restated(a, w, bias, res), want, a, w, bias, res), e32)
        ms = {m: O.ratio("gemm", O.gemm_err(O.gemm_restated(a, w, bias, res, m), want, a, w, bias, res), e32) for m in O.GEMM_MUTANTS}
        print(f"gemm {shape} bias={hb} res={hr}: e32 {e32 / O.U:.2f} u, restatement {r:.2f} x, mutants", {m: round(v, 2) for m, v in ms.items()})
        assert r <= O.FACTOR["gemm"] / 2, (shape, hb, hr, r)
        for m, v in ms.items():
            if v > worst[m][0]:
                worst[m] = (v, (shape, hb, hr))
            if shape == (65, 64, 4096) and not hb and not hr:          # the stage-1 sr conv's products alone: teeth under the floor
                assert v > TEETH * O.FACTOR["gemm"], (m, v)
    check_teeth("gemm", worst, O.GEMM_MUTANTS)


def test_gemm_special_cases_are_what_they_claim():
    a, w = O.gemm_special("midlo")
    hi = a.to(torch.bfloat16).float()
    assert torch.all(hi == 1) and float((a - hi).abs().max()) > 0          # all the information is below the hi part
    assert torch.all((hi @ w.t()) == 0)                                    # and the hi.hi products cancel
    want = O.gemm(a.double(), w.double())
    assert float(want.abs().min()) > 0
    lost = O.gemm_err((a - hi - (a - hi).to(torch.bfloat16).float()) @ w.t(), 0 * want, a, w)      # what the lo part carries
    assert lost > TEETH * O.FACTOR["gemm"] * O.FLOOR["gemm"], lost          # enough for the bound to miss it
    a, w = O.gemm_special("zero rows")
    want = O.gemm(a.double(), w.double())
    assert torch.all(want[[3, 64, 65, 66]] == 0) and torch.all(want[:, [0, 69]] == 0) and float(want[0, 1].abs()) > 0


def test_layernorm_restatement_and_mutants():
    worst = {m: (0.0, None) for m in O.LN_MUTANTS}
    for c, eps in sorted({(c, eps) for c, eps, _ in O.LN_CASES}):
        x, g, b = O.layernorm_inputs(c)
        want = O.layernorm(*d(x, g, b), eps)
        got32, floor = O.fp32(O.layernorm, x, g, b, eps), O.layernorm_floor(x)
        r = O.token_ratio(O.layernorm_restated(x, g, b, eps), got32, want, floor)
        ms = {m: O.token_ratio(O.layernorm_restated(x, g, b, eps, m), got32, want, floor) for m in O.LN_MUTANTS}
        print(f"layernorm C={c} eps={eps}: e32 per token / u {np.round(O.token_errs(got32, want) / O.U, 1)}, floor / u "
              f"{np.round(floor / O.U, 1)}, restatement {r:.2f} x, mutants", {m: float(f"{v:.3g}") for m, v in ms.items()})
        assert r <= O.FACTOR["layernorm"] / 2, (c, eps, r)
        assert torch.equal(want[O.LN_ZERO_TOKEN], b.double())
        for m, v in ms.items():
            if v > worst[m][0]:
                worst[m] = (v, (c, eps))
    check_teeth("layernorm", worst, O.LN_MUTANTS)


def test_attention_restatement_and_mutants():
    worst = {m: (0.0, None) for m in O.AT_MUTANTS}
    for case in O.AT_SHAPES + O.AT_SPECIAL:
        q, kv = O.attention_special(case) if isinstance(case, str) else O.attention_inputs(*case)
        want = O.attention(*d(q, kv), O.AT_SCALE)
        e32 = O.attention_err(O.fp32(O.attention, q, kv, O.AT_SCALE), want, kv)
        got = O.attention_restated(q, kv, O.AT_SCALE)
        r = O.ratio("attention", O.attention_err(got, want, kv), e32)
        ms = {m: O.ratio("attention", O.attention_err(O.attention_restated(q, kv, O.AT_SCALE, m), want, kv), e32) for m in O.AT_MUTANTS}
        print(f"attention {case}: e32 {e32 / O.U:.2f} u, restatement {r:.2f} x, mutants", {m: float(f"{v:.3g}") for m, v in ms.items()})
        assert r <= O.FACTOR["attention"] / 2, (case, r)
        assert bool(torch.isfinite(got).all())
        if kv.shape[0] == 1:
            assert torch.equal(got, kv[:, q.shape[1]:].expand(q.shape[0], -1))          # p = 1, l = 1: the V row, bit for bit
        for m, v in ms.items():
            if v > worst[m][0]:
                worst[m] = (v, case)
    check_teeth("attention", worst, O.AT_MUTANTS)


def test_attention_special_cases_are_what_they_claim():
    q, kv = O.attention_special("peaked")
    s = (q.double() @ kv[:, :64].double().t()) * O.AT_SCALE
    assert float(s.max()) == 90.0 and float(s.min()) < -85.0
    top = s.argmax(dim=1) // O.AT_KEYS
    assert top.tolist() == [0] * 16 + [1] * 16 + [2] * 16 + [0] * 16
    first = s[:, :16].max(dim=1).values
    assert torch.all(first[16:32] == 50) and torch.all(first[32:48] == 30)
    second = torch.sort(s[48:], dim=1, descending=True).values[:, 1]
    assert torch.all(second == 90.0 - 2.0 ** -10) and torch.all(s[48:, 32:].max(dim=1).values == second)
    q, kv = O.attention_special("identical keys")
    want = O.attention(q.double(), kv.double(), O.AT_SCALE)
    assert float((want - kv[:, 64:].double().mean(dim=0)).abs().max()) < 1e-14


def test_gross_faults_of_the_plain_kernels_exceed_their_bounds():
    """dwconv + GELU and the head sum have no restatement: their faults are gross.  The bounds still have to see them."""
    worst = {"tanh GELU": 0.0, "transposed taps": 0.0, "wrapped border": 0.0}
    for h, w, c in O.DW_CASES:
        x, wt, b = O.dwconv_inputs(h, w, c)
        xd, wd, bd = d(x, wt, b)
        want = O.dwconv_gelu(xd, wd, bd, h, w)
        got32, floor = O.fp32(O.dwconv_gelu, x, wt, b, h, w), O.dwconv_floor(x, wt, b, h, w, want)
        pre = F.conv2d(O._planar(xd, h, w), wd.t().reshape(c, 1, 3, 3), bd, padding=1, groups=c)
        wrap = F.conv2d(F.pad(O._planar(xd, h, w), (1, 1, 1, 1), mode="circular"), wd.t().reshape(c, 1, 3, 3), bd, groups=c)
        faults = {"tanh GELU": F.gelu(O._tokens(pre), approximate="tanh"),
                  "transposed taps": O.dwconv_gelu(xd, wd.reshape(3, 3, c).transpose(0, 1).reshape(9, c), bd, h, w),
                  "wrapped border": F.gelu(O._tokens(wrap))}
        for k, got in faults.items():
            worst[k] = max(worst[k], O.token_ratio(got, got32, want, floor))
    print("dwconv + GELU faults:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert min(worst.values()) > TEETH * O.FACTOR["dwconv_gelu"]
    for gi, grids in enumerate(O.HEAD_GRIDS):
        ys = O.head_inputs(gi)
        want = O.head_sum(d(*ys), grids)
        got32, floor = O.fp32(O.head_sum, ys, grids), O.head_floor(ys, grids, want)
        acc = O._planar(ys[0].double(), *grids[0])
        for y, g in zip(ys[1:], grids[1:]):
            acc = acc + F.interpolate(O._planar(y.double(), *g), size=grids[0], mode="bilinear", align_corners=True)
        r = O.token_ratio(O._tokens(F.relu(acc)), got32, want, floor)
        print(f"head sum grids {gi}: align_corners=True is {r:.3g} x")
        assert r > TEETH * O.FACTOR["head_sum"]


def test_references_compose_into_the_networks_blocks():
    """gemm -> LN -> attention -> ... from the fp64 op references and the LIBRARY's tensor layouts equals segformer_ref's block:
    K order (ky, kx, c) of both gathers, kv columns (K at 64 h, V at C + 64 h), dw weights [9][C]."""
    from vstnet_amd.segformer import fold_decode_head, library_tensors
    from vstnet_amd.synth import synthetic_segformer_state_dict
    depths = (1, 1, 1, 1)
    sd32 = synthetic_segformer_state_dict(4321, depths)
    sd = R.cast(sd32, torch.float64)
    lt = {k: torch.from_numpy(v).double() for k, v in library_tensors(sd32, depths).items()}
    g = torch.Generator().manual_seed(11)

    def close(a, b):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())), float((a - b).abs().max())
    # stage 2: C = 128, two heads, sr = 4 on an 8 x 12 grid (6 keys)
    c, h, w, sr = 128, 8, 12, 4
    x = torch.randn((h * w, c), generator=g, dtype=torch.float64)
    p = "backbone.block2.0.attn."
    q = O.gemm(x, lt[p + "q.weight"].reshape(c, c), lt[p + "q.bias"])
    col = O.im2col(x, h, w, sr, sr, 0)
    red = O.layernorm(O.gemm(col, lt[p + "sr.weight"].reshape(c, sr * sr * c), lt[p + "sr.bias"]), lt[p + "norm.weight"], lt[p + "norm.bias"], 1e-5)
    kv = O.gemm(red, lt[p + "kv.weight"].reshape(2 * c, c), lt[p + "kv.bias"])
    y = O.gemm(O.attention(q, kv, 0.125), lt[p + "proj.weight"].reshape(c, c), lt[p + "proj.bias"], res=x)
    close(y, x + R._attention(x, h, w, sd, p, 2, sr))
    p = "backbone.block2.0.mlp."
    h1 = O.gemm(x, lt[p + "fc1.weight"].reshape(4 * c, c), lt[p + "fc1.bias"])
    h2 = O.dwconv_gelu(h1, lt[p + "dwconv.dwconv.weight"].reshape(9, 4 * c), lt[p + "dwconv.dwconv.bias"], h, w)
    close(O.gemm(h2, lt[p + "fc2.weight"].reshape(c, 4 * c), lt[p + "fc2.bias"]), R._mlp(x, h, w, sd, p))
    # both gathers against the convs: patch_embed1 from a 70 x 101 frame (replicate-padded to 72 x 104), patch_embed2 from its map
    frame = O.rgb_frame(70, 101)
    rows, _ = O.gather_rgb(frame)
    x1 = O.gemm(rows, lt["backbone.patch_embed1.proj.weight"].reshape(64, 147), lt["backbone.patch_embed1.proj.bias"])
    f = F.pad(frame.permute(2, 0, 1)[None].double() / 255.0, (0, 3, 0, 2), mode="replicate")
    f = (f - torch.tensor(R.MEAN, dtype=torch.float64).reshape(1, 3, 1, 1)) / torch.tensor(R.STD, dtype=torch.float64).reshape(1, 3, 1, 1)
    m1 = F.conv2d(f, sd["backbone.patch_embed1.proj.weight"], sd["backbone.patch_embed1.proj.bias"], stride=4, padding=3)
    assert m1.shape[2:] == (18, 26)
    close(x1, O._tokens(m1))
    x2 = O.gemm(O.im2col(x1, 18, 26, 3, 2, 1), lt["backbone.patch_embed2.proj.weight"].reshape(128, 576), lt["backbone.patch_embed2.proj.bias"])
    close(x2, O._tokens(F.conv2d(m1, sd["backbone.patch_embed2.proj.weight"], sd["backbone.patch_embed2.proj.bias"], stride=2, padding=1)))
    # the folded head's upsample-sum
    grids = O.HEAD_GRIDS[0]
    xs = [torch.randn((cc, gh, gw), generator=g, dtype=torch.float64) for cc, (gh, gw) in zip(R.DIMS, grids)]
    folded = {k: torch.from_numpy(v) for k, v in fold_decode_head(sd).items()}
    ys = [O.gemm(O._tokens(xm[None]), folded[f"fold_c{i + 1}.weight"], folded["fold.bias"] if i == 0 else None) for i, xm in enumerate(xs)]
    lg = O.gemm(O.head_sum(ys, grids), sd["decode_head.linear_pred.weight"].reshape(150, -1), sd["decode_head.linear_pred.bias"])
    close(lg, O._tokens(R.folded_head(folded, sd, xs)[None]))


def test_gather_rgb_reference_marks_the_zero_padding():
    rows, pad = O.gather_rgb(O.rgb_frame(70, 101))
    assert rows.shape == (18 * 26, 147) and bool((rows[pad] == 0).all()) and float(rows[~pad].abs().min()) > 1e-4
    assert int(pad.sum()) == 3 * (3 * 7 * 26 + 3 * 7 * 18 - 9)          # three rows above, three columns left; nothing below / right


def test_kernel_level_calls_are_declared_exported_and_built():
    from vstnet_amd import _lib
    from vstnet_amd import segformer
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name in _lib.EXPORTS, name
        assert callable(getattr(segformer.ops, name[len("vst_seg_"):]))
    assert "kernel-level call" in hdr.lower()
    L = built_library()
    assert L.vst_version() >= 111
    for name in NAMES:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name


def test_refusals_need_no_gpu():
    """Every refusal comes before any launch, so the argument checks answer on a machine without a GPU too."""
    import ctypes as C
    from vstnet_amd import _lib
    L = built_library()
    ok, off, null = C.c_void_p(4096), C.c_void_p(4096 + 4), C.c_void_p(0)
    assert L.vst_seg_gemm(null, ok, null, null, ok, 1, 1, 1, null) == -1
    assert L.vst_seg_gemm(ok, ok, off, null, ok, 1, 1, 1, null) == -1
    assert L.vst_seg_gemm(ok, ok, null, null, ok, 0, 1, 1, null) == -2
    assert L.vst_seg_layernorm(ok, ok, ok, ok, 5, 513, 1e-5, null) == -2
    assert L.vst_seg_attention(ok, ok, ok, 5, 5, 96, 0.125, null) == -2
