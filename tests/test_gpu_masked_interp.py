"""GPU: style interpolation under masks (several styles and alpha_c per label).  The reduction to one style is the masked
transfer bit for bit on every route, and both equal the transfer composed by hand from the single-style entry points of the
library (tests/masked_legacy_ref.py), plan tables and affines included; prefactored bindings give the raw records' affines bit for bit; the mixes agree with the
oracle composed from cpu_ref.compute_label_info + cpu_ref.interpolation (tests/masked_interp_ref.py) within the tolerances the
existing tests use for the same routes; the drivers honour the new flags."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import cpu_ref
from tests import masked_legacy_ref as legacy
from tests.masked_interp_ref import interpolation_seg_ref, region_mask
from vstnet_amd.code import from_dense
from vstnet_amd.synth import synthetic_state_dict, synthetic_frames

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def rel(got, ref):
    d = got.detach().cpu().double() - ref.double()
    return float(d.norm() / ref.double().norm()), float(d.abs().max() / ref.double().abs().max())


def codes(N, B, K, seed, chw=(96, 256), shw=(80, 240)):
    """well-conditioned codes: a fixed channel mixer on white noise (its strength falls with N so that the mixer's spectrum stays
    away from zero), another scale and offset per style"""
    g = torch.Generator().manual_seed(seed)
    mixer = torch.eye(N) + 0.25 * min(1.0, (32 / N) ** 1.5) * torch.randn(N, N, generator=g)
    mk = lambda h, w, k: torch.einsum("ij,bjhw->bihw", mixer, torch.randn(B, N, h, w, generator=g)) * (0.5 + 0.2 * k) + 0.1 * k
    return mk(*chw, 0), [mk(shw[0], shw[1] - 16 * k, k + 1) for k in range(K)]


def maps(B, K, seed, chw=(96, 256), shw=(80, 240)):
    """3 labels of >= 6000 pixels each in every map, different maps per sample; label 2 is missing (6 pixels) from the LAST
    style's map of sample 0 only: valid for the other styles, so its pixels must keep the content bits there."""
    cm = np.stack([region_mask(*chw, [0, 1, 2], seed + b) for b in range(B)])
    sms = []
    for k in range(K):
        per = []
        for b in range(B):
            hw = (shw[0], shw[1] - 16 * k)
            per.append(region_mask(*hw, [0, 1], seed + 10 * k + b, tiny=2) if (k == K - 1 and b == 0)
                       else region_mask(*hw, [0, 1, 2], seed + 10 * k + b))
        sms.append(np.stack(per))
    return cm, sms


def one_style_case(N, B=2, seed=3):
    c, (s,) = codes(N, B, 1, seed)
    cm = np.stack([region_mask(96, 256, [0, 1, 2], seed + b, tiny=3) for b in range(B)])
    sm = np.stack([region_mask(80, 240, [0, 1, 2], seed + 5 + b) for b in range(B)])
    return c.cuda(), s.cuda(), cm, sm


# ------------------------------------------------------------------------------------------- 1. bit identity with one style
@pytest.mark.parametrize("N", [32, 128])
def test_one_style_is_the_masked_transfer_single_pass(N):
    from models.cWCT import cWCT
    cw = cWCT()
    c, s, cm, sm = one_style_case(N)
    ref = cw.transfer(c, s, cm, sm)
    assert cw.last_route == "masked_single_pass"
    got = cw.interpolation(c, [s], [1.0], 0.0, cm, [sm])
    assert cw.last_route == "interp_masked_single_pass"
    assert torch.equal(got, ref) and not torch.equal(got, c)
    info = cw.last_info.reshape(32, 3).cpu()
    assert int(info[:3, 1].abs().sum()) == 0
    # third side: vst_label_plan + vst_cwct_stats_labels + vst_cwct_factor_labels + vst_cwct_apply_labels, called by hand
    want, tables, affines = legacy.transfer_single_pass(c, s, cm, sm, cw.precision)
    assert torch.equal(ref, want) and torch.equal(got, want)
    plan = cw.plan_masks(cm, sm, c.shape, s.shape, c.device)
    # (the codes of one_style_case are einsum results with the sample axis second in memory: made NCHW before pointers are taken)
    c2, s2, rec = c.contiguous().reshape(2, N, -1), s.contiguous().reshape(2, N, -1), N * N + N
    for b in range(2):
        assert torch.equal(plan.tables[b], tables[b])                   # the builder's table == vst_label_plan's, every byte
        labels = legacy.assert_table_is_the_numpy_plan(plan.tables[b], cm[b], [sm[b]])
        assert len(labels) == 3 and labels == cw.plan_info(plan, b)[0]
        aff, finfo = torch.empty(32 * rec, device="cuda"), torch.empty(32 * 3, dtype=torch.int32, device="cuda")
        cw._factor_labels(cw._stats_labels(c2[b], plan.cm[b], plan.tables[b], 0),
                          [cw._stats_labels(s2[b], plan.sms[0][b], plan.tables[b], 0)], plan.tables[b], None, [1.0], 0.0, 0, N, aff, finfo)
        assert torch.equal(aff[:3 * rec], affines[b][:3 * rec]) and float(aff[:3 * rec].abs().sum()) > 0


def test_one_style_is_the_masked_transfer_packed_rows():
    from models.cWCT import cWCT
    cw = cWCT()
    c, s, cm, sm = one_style_case(32)
    z = from_dense(c)
    plan = cw.learn_slots(cw.plan_masks(cm, sm, z.shape, s.shape, z.device))
    ref = cw.transfer_with_plan(z, s, plan)
    assert cw.last_route == "masked_packed_rows" and ref.pending
    got = cw.interpolation(from_dense(c), [s], [1.0], 0.0, cm, [sm])
    assert cw.last_route == "interp_masked_packed_rows" and got.pending
    for b in range(2):
        assert torch.equal(got.pending_labels[0][b][0][:3 * 1056], ref.pending_labels[0][b][0][:3 * 1056])
    assert torch.equal(got.materialize(), ref.materialize())
    # third side: vst_label_plan + vst_cwct_stats_labels_code / _labels + vst_cwct_factor_labels, called by hand
    assert plan.max_slots == 3
    want, tables, affines = legacy.transfer_packed_rows(from_dense(c), s, cm, sm, plan.max_slots)
    for b in range(2):
        assert torch.equal(plan.tables[b], tables[b])
        assert len(legacy.assert_table_is_the_numpy_plan(plan.tables[b], cm[b], [sm[b]])) == 3
        assert torch.equal(ref.pending_labels[0][b][0][:3 * 1056], affines[b][:3 * 1056])
        assert torch.equal(ref.pending_labels[0][b][1], want.pending_labels[0][b][1])      # the map in the rows' order
    assert torch.equal(ref.materialize(), want.materialize()) and not torch.equal(want.materialize(), c)


@pytest.mark.parametrize("N", [16, 24])
def test_one_style_is_the_masked_transfer_per_label(N):
    from models.cWCT import cWCT
    cw = cWCT()
    c, s, cm, sm = one_style_case(N)
    ref = cw.transfer(c, s, cm, sm)
    got = cw.interpolation(c, [s], [1.0], 0.0, cm, [sm])
    assert cw.last_route == "interp_masked_per_label"
    assert torch.equal(got, ref) and not torch.equal(got, c)
    want = legacy.transfer_per_label(cw, c, s, cm, sm)        # third side: the reference's loop from cw.stats / factor / apply
    assert torch.equal(ref, want) and torch.equal(got, want)


def test_one_style_is_the_masked_transfer_f64():
    from models.cWCT import cWCT
    cw = cWCT(use_double=True)
    c, s, cm, sm = one_style_case(32)
    ref = cw.transfer(c, s, cm, sm)
    got = cw.interpolation(c, [s], [1.0], 0.0, cm, [sm])
    assert cw.last_route == "interp_masked_per_label" and torch.equal(got, ref)
    want = legacy.transfer_per_label(cw, c, s, cm, sm)        # third side: the reference's loop from the fp64 calls
    assert torch.equal(ref, want) and torch.equal(got, want) and not torch.equal(want, c)


@pytest.mark.parametrize("cap", [8, 32])
def test_one_style_is_the_keyed_per_frame_transfer(cap):
    from models.cWCT import cWCT
    cw = cWCT()
    c, s, cm, sm = one_style_case(32, B=1)
    z = from_dense(c) if cap == 8 else c
    binding = cw.bind_style_labels(s, sm[0])
    mask = T(cm[0]).cuda()
    plan = cw.plan_frame(mask, binding, max_slots=cap)
    ref = cw.transfer_with_plan(z, None, plan)
    got = cw.transfer_with_plan(z, None, cw.plan_frame(mask, [binding], max_slots=cap), alpha_s=[1.0], alpha_c=0.0)
    assert cw.last_route == ("interp_masked_packed_rows" if cap == 8 else "interp_masked_single_pass")
    dense = lambda t: t.materialize() if cap == 8 else t      # noqa: E731
    assert torch.equal(dense(got), dense(ref)) and not torch.equal(dense(got), c)
    assert torch.equal(dense(got), cw.transfer(c, s, cm, sm)) or cap == 8      # the keyed route == the plain one (dense applies)
    # third side: vst_label_plan_hist (style map against itself, frame against the style) + vst_cwct_factor_labels_keyed, by hand
    want, table, aff = legacy.transfer_keyed_frame(from_dense(c) if cap == 8 else c, s[0], cm[0], sm[0], cap, cw.precision)
    assert torch.equal(plan.tables[0], table)
    assert len(legacy.assert_table_is_the_numpy_plan(plan.tables[0], cm[0], [sm[0]], cap)) == 3
    assert torch.equal(dense(ref), dense(want)) and torch.equal(dense(got), dense(want))
    if cap == 8:
        assert torch.equal(ref.pending_labels[0][0][0][:3 * 1056], aff[:3 * 1056]) and float(aff[:3 * 1056].abs().sum()) > 0


# ------------------------------------------------------------------------------------------- 2. prefactored bindings
def test_prefactored_records_give_the_same_affines():
    from models.cWCT import cWCT
    cw = cWCT()
    c, styles = codes(32, 1, 2, 11)
    cm, sms = maps(1, 2, 11)
    c, styles = c.cuda(), [s.cuda() for s in styles]
    z = from_dense(c)
    shapes = [s.shape for s in styles]
    out = {}
    for pre in (False, True):
        plan = cw.bind_style(cw.learn_slots(cw.plan_masks(cm, sms, z.shape, shapes, z.device)), styles, prefactor=pre)
        assert (float(plan.styles[0][0][0]) < 0) == pre                 # prefactored records carry -(n+1)
        t = cw.transfer_with_plan(z, None, plan, alpha_s=[0.6, 0.4], alpha_c=0.3)
        n = len(cw.plan_info(plan)[0])
        out[pre] = (t.pending_labels[0][0][0][:n * 1056].clone(), t.materialize())
        bind = cw.bind_style_labels(styles, [m[0] for m in sms], prefactor=pre)
        t = cw.transfer_with_plan(z, None, cw.plan_frame(T(cm[0]).cuda(), bind, max_slots=8), alpha_s=[0.6, 0.4], alpha_c=0.3)
        out[pre] += (t.pending_labels[0][0][0][:n * 1056].clone(),)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert torch.equal(out[True][2], out[False][2])
    assert torch.equal(out[True][2], out[True][0])                       # keyed bindings == records in the plan's slot order


# ------------------------------------------------------------------------------------------- 3. against the composed oracle
# tolerances: the project's existing ones for the same routes (rel-L2 / max-rel)
ROUTE_CASES = [("single_pass", 32, 2e-4, 1e-3), ("single_pass", 128, 2e-4, 1e-3), ("packed_rows", 32, 2e-4, 1e-3),
               ("per_label", 16, 5e-4, 5e-3), ("per_label", 24, 5e-4, 5e-3), ("f64", 32, 2e-6, 2e-6)]


@pytest.mark.parametrize("K,ac", [(2, 0.0), (2, 0.3), (3, 0.0), (3, 0.3)])
@pytest.mark.parametrize("route,N,tol,tol_max", ROUTE_CASES, ids=[f"{r}-{n}" for r, n, _, _ in ROUTE_CASES])
def test_mix_against_the_composed_oracle(route, N, tol, tol_max, K, ac):
    from models.cWCT import cWCT
    alphas = [0.6, 0.4] if K == 2 else [0.5, 0.3, 0.2]
    c, styles = codes(N, 2, K, 100 + N)
    cm, sms = maps(2, K, 7)
    ref = interpolation_seg_ref(c, styles, alphas, ac, cm, sms, use_double=(route == "f64"))
    ref64 = interpolation_seg_ref(c.double(), [s.double() for s in styles], alphas, ac, cm, sms).float()
    own = rel(ref, ref64)
    print(f"oracle fp32 vs fp64: rel-L2 {own[0]:.2e} max-rel {own[1]:.2e}")
    assert own[0] <= tol / 10 and own[1] <= tol_max / 10 or route == "f64"
    cw = cWCT(use_double=(route == "f64"))
    cg = c.cuda()
    got = cw.interpolation(from_dense(cg) if route == "packed_rows" else cg, [s.cuda() for s in styles], alphas, ac, cm, sms)
    assert cw.last_route == {"single_pass": "interp_masked_single_pass", "packed_rows": "interp_masked_packed_rows",
                             "per_label": "interp_masked_per_label", "f64": "interp_masked_per_label"}[route]
    got = got.materialize() if route == "packed_rows" else got
    l2, mx = rel(got, ref)
    print(f"{route} N={N} K={K} alpha_c={ac}: rel-L2 {l2:.3e} max-rel {mx:.3e} (tol {tol:g}/{tol_max:g})")
    assert l2 <= tol and mx <= tol_max
    keep = T(cm[0] == 2)                         # sample 0: label 2 is invalid for the last style only
    assert int(keep.sum()) >= 6000
    assert torch.equal(got[0][:, keep].cpu(), c[0][:, keep])
    assert not torch.equal(got[1][:, T(cm[1] == 2)].cpu(), c[1][:, T(cm[1] == 2)])       # sample 1 mixes it


def test_cached_stats_mix_equals_interpolation():
    """transfer_with_stats with K styles' cached (prefactored) stats == interpolation, dense and on packed rows"""
    from models.cWCT import cWCT
    cw = cWCT()
    c, styles = codes(32, 1, 3, 21)
    c, styles = c.cuda(), [s.cuda() for s in styles]
    stats = [cw.style_stats(s) for s in styles]
    al = [0.5, 0.3, 0.2]
    assert torch.equal(cw.transfer_with_stats(c, stats, 0.3, alpha_s=al), cw.interpolation(c, styles, al, 0.3))
    a, b = cw.transfer_with_stats(from_dense(c), stats, 0.3, alpha_s=al), cw.interpolation(from_dense(c), styles, al, 0.3)
    assert cw.last_route == "packed_rows" and torch.equal(a.pending_affines, b.pending_affines)


# ------------------------------------------------------------------------------------------- 4. end to end
def make_net(precision=None):
    from models.RevResNet import RevResNet
    net = RevResNet(hidden_dim=16, sp_steps=2, precision=precision)
    sd = synthetic_state_dict(1234, 16, 2)
    net.load_state_dict(sd)
    return net.to("cuda").eval(), sd


def test_masked_two_style_stylisation_vs_oracle():
    """encode, masked 2-style interpolation, decode against cpu_ref; tolerance of test_masked_stylisation_vs_oracle (bf16x3)"""
    from models.cWCT import cWCT
    net, sd = make_net()
    cw = cWCT()
    H, W = 96, 192
    xc, xa, xb = synthetic_frames(1, H, W, seed=21), synthetic_frames(1, 96, 192, seed=22), synthetic_frames(1, 96, 160, seed=23)
    cm = region_mask(H, W, [0, 1, 2], 3, tiny=3)[None]
    sma, smb = region_mask(96, 192, [0, 1, 2], 4)[None], region_mask(96, 160, [0, 1, 2], 5)[None]
    with torch.no_grad():
        zc, za, zb = (cpu_ref.revnet_forward(x, sd, 2) for x in (xc, xa, xb))
        zcs = interpolation_seg_ref(zc, [za, zb], [0.7, 0.3], 0.3, cm, [sma, smb])
        sty = cpu_ref.revnet_inverse(zcs, sd, 2)
        g_zcs = cw.interpolation(net(xc.cuda()), [net(xa.cuda()), net(xb.cuda())], [0.7, 0.3], 0.3, cm, [sma, smb])
        assert cw.last_route == "interp_masked_packed_rows"
        g_sty = net(g_zcs, forward=False)
    for what, got, ref in (("z_cs", g_zcs, zcs), ("stylized", g_sty, sty)):
        l2, mx = rel(got.materialize() if hasattr(got, "materialize") else got, ref)
        print(f"masked 2-style {what}: rel-L2 {l2:.3e} max-rel {mx:.3e}")
        assert l2 <= 2e-4 and mx <= 1e-3, what


def _png(path, h, w, seed):
    a = (synthetic_frames(1, h, w, seed=seed)[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    Image.fromarray(a).save(path)
    return a


def test_video_cross_fade_per_frame_maps_and_shards(tmp_path):
    import video_transfer
    from models.cWCT import cWCT
    H, W, n = 64, 96, 5
    fd, sd_ = tmp_path / "clip", tmp_path / "segs"
    fd.mkdir()
    sd_.mkdir()
    frames = [_png(fd / f"{i:03d}.png", H, W, 30 + i) for i in range(n)]
    cms = [region_mask(H, W, [0, 1], 40 + i) for i in range(n)]
    for i, m in enumerate(cms):
        Image.fromarray(m, mode="L").save(sd_ / f"{i:03d}.png")
    sa, sb = _png(tmp_path / "a.png", 64, 96, 7), _png(tmp_path / "b.png", 48, 80, 8)
    sma, smb = region_mask(64, 96, [0, 1], 9), region_mask(48, 80, [0, 1], 10)
    Image.fromarray(sma, mode="L").save(tmp_path / "sa.png")
    Image.fromarray(smb, mode="L").save(tmp_path / "sb.png")
    base = ["--video", str(fd), "--styles", str(tmp_path / "a.png"), str(tmp_path / "b.png"), "--alpha_s", "0.9", "0.1",
            "--alpha_s_end", "0.2", "0.8", "--alpha_c", "0.25", "--content_seg_dir", str(sd_), "--style_segs", str(tmp_path / "sa.png"),
            str(tmp_path / "sb.png"), "--interpolate_labels", "--synthetic_weights", "--frames_only"]
    one = video_transfer.main(base + ["--out_dir", str(tmp_path / "o1")])
    weights = dict(video_transfer.LAST_RUN["weights"])
    assert sorted(os.listdir(one)) == [f"{i:05d}.png" for i in range(n)] and video_transfer.LAST_RUN["redo"] == 0
    for k in range(2):
        two = video_transfer.main(base + ["--out_dir", str(tmp_path / "o2"), "--shard", f"{k}/2"])
    for i in range(n):                   # two shards == one process, byte for byte
        assert open(os.path.join(one, f"{i:05d}.png"), "rb").read() == open(os.path.join(two, f"{i:05d}.png"), "rb").read(), i
    # frame i == the library call with frame i's weights
    net, _ = make_net()
    cw = cWCT()
    u8 = lambda a: T(np.ascontiguousarray(a))[None].cuda()      # noqa: E731
    with torch.no_grad():
        bind = cw.bind_style_labels([net.forward_u8(u8(sa)), net.forward_u8(u8(sb))], [sma, smb])
        outs = []
        for i in range(n):
            t = i / (n - 1)
            w = [(1 - t) * 0.9 + t * 0.2, (1 - t) * 0.1 + t * 0.8]
            assert weights[i] == w
            z = cw.transfer_with_plan(net.forward_u8(u8(frames[i])), None, cw.plan_frame(T(cms[i]).cuda(), bind, max_slots=8),
                                      alpha_s=w, alpha_c=0.25)
            outs.append(net.inverse_u8(z)[0].cpu().numpy())
    for i in range(n):
        assert np.array_equal(np.asarray(Image.open(os.path.join(one, f"{i:05d}.png"))), outs[i]), i
    assert not np.array_equal(outs[0], outs[-1])


def test_tiled_masks_with_alpha_c():
    """masks + alpha_c per label: tiled == whole frame within the bound tests/test_gpu_tiled.py uses for masked frames (1e-5,
    exact fp32 applies on both sides), and alpha_c really acts"""
    from models.cWCT import cWCT
    from vstnet_amd import tiled
    from vstnet_amd.synth import synthetic_mask
    net, _ = make_net()
    cw = cWCT(precision="fp32")
    H, W = 1536, 1024
    u8f = lambda h, w, s: (synthetic_frames(1, h, w, seed=s)[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)      # noqa: E731
    content, style = u8f(H, W, 11), u8f(768, 512, 12)
    cseg, sseg = synthetic_mask(H, W, labels=5, seed=3), synthetic_mask(768, 512, labels=5, seed=4)
    kw = dict(content_seg=cseg, style_seg=sseg, alpha_c=0.3, out_float=True)
    whole = tiled.stylize_whole(net, cw, content, style, interpolate_labels=True, **kw)
    info = {}
    got = tiled.stylize_tiled(net, cw, content, style, tile=512, info=info, interpolate_labels=True, **kw)
    assert info["tiles"] == 6 and info["route"] == "masked_packed_rows"
    d = float(np.abs(got - whole).max() / np.abs(whole).max())
    print(f"tiled masks + alpha_c vs whole frame: max-rel {d:.3e}")
    assert d <= 1e-5
    ignored = tiled.stylize_whole(net, cw, content, style, **kw)             # without the keyword: alpha_c ignored, as before
    assert np.array_equal(ignored, tiled.stylize_whole(net, cw, content, style, content_seg=cseg, style_seg=sseg, out_float=True))
    assert float(np.abs(whole - ignored).max()) > 1e-3
