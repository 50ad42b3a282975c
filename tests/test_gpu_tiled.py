"""GPU: halo-tiled stylisation (vstnet_amd/tiled.py) - the receptive radius is safe and tight, the rectangle statistics equal
the statistics of the sliced code, the tiled driver equals the whole-frame path, and frames past the whole-frame guard are
stylised in tiles with seams and corners that match the whole-frame arithmetic and the oracle."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from vstnet_amd import _lib, tiled
from vstnet_amd.synth import synthetic_state_dict, synthetic_mask

pytestmark = pytest.mark.gpu


def make_net(mode="photo", precision="bf16x3"):
    from models.RevResNet import RevResNet
    hd, sp = (16, 2) if mode == "photo" else (64, 1)
    net = RevResNet(hidden_dim=hd, sp_steps=sp, precision=precision)
    sd = synthetic_state_dict(1234, hd, sp)
    net.load_state_dict(sd)
    return net.to("cuda").eval(), sd, sp


def u8_frame(H, W, seed):
    """A synthetic photo: 64 x 64 blocks of random colour plus pixel noise (uint8 HWC, host; cheap at 16384 x 16384)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 192, size=(H // 64 + 1, W // 64 + 1, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 64, axis=0)[:H], 64, axis=1)[:, :W]
    return img + rng.integers(0, 64, size=(H, W, 3), dtype=np.uint8)


def _foot_dist(c, p, foot):
    """Distance along one axis between code pixels c (frame footprint [foot c, foot c + foot - 1]) and frame pixel p."""
    return np.maximum(np.maximum(foot * c - p, p - (foot * c + foot - 1)), 0)


# ------------------------------------------------------------------------------------------------ 1. radius
@pytest.mark.parametrize("mode", ["photo", "art"])
def test_receptive_radius_is_safe_and_tight(mode):
    net, _, sp = make_net(mode)
    foot = 1 if sp == 2 else 2
    x = torch.from_numpy(u8_frame(1024, 1024, 3)).cuda()[None]
    with torch.no_grad():
        # forward: one frame pixel
        r_f = tiled.receptive_radius(net, "forward")
        py, px = 509, 514
        x2 = x.clone()
        x2[0, py, px] = 255 - x2[0, py, px]
        z0, z1 = net.forward_u8(x).materialize(), net.forward_u8(x2).materialize()
        changed = (z0 != z1).any(dim=1)[0].cpu().numpy()
        cy, cx = np.nonzero(changed)
        d = np.maximum(_foot_dist(cy, py, foot), _foot_dist(cx, px, foot))
        assert d.max() <= r_f, f"forward reaches {d.max()} > radius {r_f}"
        assert d.max() >= r_f - 16, f"forward radius {r_f} is loose: reached {d.max()}"
        # inverse: one code pixel
        r_i = tiled.receptive_radius(net, "inverse")
        qy, qx = (509, 514) if sp == 2 else (253, 258)
        z2 = z0.clone()
        z2[0, :, qy, qx] += 64.0
        y0, y1 = net(z0, forward=False), net(z2, forward=False)
        changed = (y0 != y1).any(dim=1)[0].cpu().numpy()
        fy, fx = np.nonzero(changed)
        d = np.maximum(_foot_dist(qy, fy, foot), _foot_dist(qx, fx, foot))
        assert d.max() <= r_i, f"inverse reaches {d.max()} > radius {r_i}"
        # The cone's last pixels are reached only through the corner taps of ~30 convs in a row, whose product falls below fp32
        # rounding of the frame: the measured reach stops 17 (photo) / 32 (artistic) pixels short ("Ultra-resolution")
        assert d.max() >= r_i - 40, f"inverse radius {r_i} is loose: reached {d.max()}"


# ------------------------------------------------------------------------------------------------ 2. rectangle statistics
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("mode", ["photo", "art"])
def test_rect_stats_equal_stats_of_the_sliced_code(mode):
    from models.cWCT import cWCT
    net, _, sp = make_net(mode)
    cw = cWCT(precision="bf16x3")
    H, W = 256, 320
    f = 1 if sp == 2 else 2
    with torch.no_grad():
        z = net.forward_u8(torch.from_numpy(u8_frame(H, W, 5)).cuda()[None])
        zd = z.materialize()
        full = tiled.stats_code_rect(cw, z.packed[0], H, W, sp, (0, 0, H, W))
        assert torch.equal(full, cw.stats_code(z, 0))                      # bit-identical to vst_cwct_stats_code
        rng = np.random.default_rng(7)
        for _ in range(6):
            h, w = int(rng.integers(1, H // 2)) * 2, int(rng.integers(1, W // 2)) * 2
            y0, x0 = int(rng.integers(0, (H - h) // 2 + 1)) * 2, int(rng.integers(0, (W - w) // 2 + 1)) * 2
            got = tiled.stats_code_rect(cw, z.packed[0], H, W, sp, (y0, x0, h, w))
            sl = zd[0, :, y0 // f:(y0 + h) // f, x0 // f:(x0 + w) // f].reshape(zd.shape[1], -1).contiguous()
            ref = cw.stats(sl)
            N = zd.shape[1]
            assert float(got[0]) == float(ref[0]) == sl.shape[1]
            assert _rel(got[1:1 + N], ref[1:1 + N]) < 1e-5 and _rel(got[1 + N:], ref[1 + N:]) < 1e-5, (y0, x0, h, w)


def test_rect_label_stats_equal_stats_of_the_sliced_code():
    from models.cWCT import cWCT
    net, _, _ = make_net("photo")
    cw = cWCT(precision="bf16x3")
    H, W = 256, 320
    mask = synthetic_mask(H, W, labels=5, seed=2)
    mask = np.asarray(mask, dtype=np.uint8).reshape(H, W)
    with torch.no_grad():
        z = net.forward_u8(torch.from_numpy(u8_frame(H, W, 6)).cuda()[None])
        zd = z.materialize()
        m = torch.from_numpy(mask).cuda().reshape(-1)
        plan, n_slots = tiled.label_plan(m, m)
        assert 1 <= n_slots <= 8
        rows = tiled.mask_rows(m, H, W)
        full = tiled.stats_labels_code_rect(cw, z.packed[0], H, W, (0, 0, H, W), rows, plan, n_slots)
        ref_full = torch.empty(cw.MAX_SLOTS * (1 + 32 + 1024), dtype=torch.float64, device="cuda")
        ws = cw._workspace(_lib.lib().vst_cwct_stats_labels_code_workspace_bytes(H, W), ref_full.device)
        _lib.check(_lib.lib().vst_cwct_stats_labels_code(tiled._ptr(z.packed[0]), H, W, tiled._ptr(rows), tiled._ptr(plan),
                                                         n_slots, tiled._ptr(ref_full), tiled._ptr(ws), tiled._stream_ptr()),
                   "vst_cwct_stats_labels_code")
        assert torch.equal(full[:n_slots], ref_full.reshape(cw.MAX_SLOTS, -1)[:n_slots])
        for (y0, x0, h, w) in [(8, 12, 100, 64), (128, 0, 128, 320), (36, 200, 52, 120)]:
            got = tiled.stats_labels_code_rect(cw, z.packed[0], H, W, (y0, x0, h, w), rows, plan, n_slots)
            sl = zd[0, :, y0:y0 + h, x0:x0 + w].reshape(32, -1).contiguous()
            ms = torch.from_numpy(np.ascontiguousarray(mask[y0:y0 + h, x0:x0 + w])).cuda().reshape(-1)
            ref = cw._stats_labels(sl, ms, plan, n_slots).reshape(cw.MAX_SLOTS, -1)
            for k in range(n_slots):
                assert float(got[k, 0]) == float(ref[k, 0])
                if float(ref[k, 0]) > 1:
                    assert _rel(got[k, 1:], ref[k, 1:]) < 1e-5, (k, y0, x0, h, w)


# ------------------------------------------------------------------------------------------------ 3. tiled = whole frame
CASES = [
    ("unmasked", dict()),
    ("masked", dict(masked=True)),
    ("alpha_c", dict(alpha_c=0.3)),
    ("luminance", dict(preserve_luminance=True)),
    ("artistic", dict(mode="art")),
    ("f16x2h", dict(precision="f16x2h")),
    ("use_double", dict(use_double=True)),
]


@pytest.mark.parametrize("name,cfg", CASES, ids=[c[0] for c in CASES])
def test_tiled_equals_whole_frame(name, cfg):
    from models.cWCT import cWCT
    net, _, _ = make_net(cfg.get("mode", "photo"), cfg.get("precision", "bf16x3"))
    # masked: the whole-frame route applies the maps on the NCHW code, by default on split bf16 operands (~1.5e-5); the tiled
    # route applies them exactly while decoding - compare both in exact fp32 applies
    cw = cWCT(precision="fp32" if cfg.get("masked") else cfg.get("precision", "bf16x3"), use_double=cfg.get("use_double", False))
    H, W = 3072, 2048
    content, style = u8_frame(H, W, 11), u8_frame(1536, 1024, 12)
    cseg = sseg = None
    if cfg.get("masked"):
        cseg = np.asarray(synthetic_mask(H, W, labels=5, seed=3), dtype=np.uint8).reshape(H, W)
        sseg = np.asarray(synthetic_mask(1536, 1024, labels=5, seed=4), dtype=np.uint8).reshape(1536, 1024)
    kw = dict(content_seg=cseg, style_seg=sseg, alpha_c=cfg.get("alpha_c"), preserve_luminance=cfg.get("preserve_luminance", False))
    whole = tiled.stylize_whole(net, cw, content, style, out_float=True, **kw)
    info = {}
    got = tiled.stylize_tiled(net, cw, content, style, tile=1024, out_float=True, info=info, **kw)
    assert info["tiles"] == 6 and info["route"] != "whole_frame"
    # (the Lab round trip of preserve_luminance roughly doubles the fp32 noise of the stylised channels)
    tol = 2e-4 if cfg.get("precision") == "f16x2h" else (2e-5 if cfg.get("preserve_luminance") else 1e-5)
    d = float(np.abs(got - whole).max() / np.abs(whole).max())
    assert d <= tol, f"{name}: tiled vs whole frame max-rel {d:.3e} (route {info['route']})"
    if name == "unmasked":                 # a tile that covers the frame IS the whole-frame path, u8 and float
        assert np.array_equal(tiled.stylize_tiled(net, cw, content, style, tile=4096, out_float=True, **kw), whole)
        assert np.array_equal(tiled.stylize_tiled(net, cw, content, style, tile=4096, **kw),
                              tiled.stylize_whole(net, cw, content, style, **kw))


# ------------------------------------------------------------------------------------------------ 4. past 2^31 bytes
def test_8192_whole_frame_vs_oracle_and_tiled():
    """8192 x 8192: the whole-frame code (8.6 GB) and decoded frame at both corners against the oracle; the tiled run (tile
    4096) against the whole-frame run, and its merged content statistics against the whole-frame statistics."""
    from models.cWCT import cWCT
    from tests.test_gpu_parity import check_corners_vs_oracle, TIGHT
    net, sd, sp = make_net("photo")
    cw = cWCT(precision="bf16x3")
    H = W = 8192
    content, style = u8_frame(H, W, 21), u8_frame(1024, 1024, 22)
    with torch.no_grad():
        xc = torch.from_numpy(content).cuda()[None]
        z = net.forward_u8(xc)
        whole_stats = cw.stats_code(z, 0)
        zcs = cw.transfer(z, net.forward_u8(torch.from_numpy(style).cuda()[None]))
        sty = net(zcs, forward=False)
        x_cpu = xc.permute(0, 3, 1, 2).float().div(255.0).cpu()
        check_corners_vs_oracle(x_cpu, z, zcs, sty, sd, sp, 5e-5, TIGHT, "8192x8192 (bf16x3)")
        whole = sty[0].permute(1, 2, 0).cpu().numpy()
        del z, zcs, sty, xc
    torch.cuda.empty_cache()
    info = {}
    got = tiled.stylize_tiled(net, cw, content, style, tile=4096, out_float=True, info=info)
    assert info["tiles"] == 4
    d = float(np.abs(got - whole).max() / np.abs(whole).max())
    assert d <= 1e-5, d
    cs = info["content_stats"]
    assert float(cs[0]) == H * W
    # (the per-workgroup sums are fp32: a different grouping of the same rows moves the record by fp32 rounding)
    assert _rel(cs[1:], whole_stats[1:]) < 1e-6


# ------------------------------------------------------------------------------------------------ 5. past the guard
def test_16384_past_the_guard_tiled():
    from models.cWCT import cWCT
    net, sd, sp = make_net("photo")
    cw = cWCT(precision="bf16x3")
    H = W = 16384
    assert H * W > tiled.max_frame_pixels()
    content, style = u8_frame(H, W, 31), u8_frame(1024, 1024, 32)
    with torch.no_grad():
        big = torch.from_numpy(content).cuda()[None]
        before = torch.cuda.memory_allocated()
        with pytest.raises(RuntimeError, match="stylize_tiled"):
            net.forward_u8(big)
        assert torch.cuda.memory_allocated() == before                 # refused before any allocation
        del big
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    info = {}
    out = tiled.stylize_tiled(net, cw, content, style, tile=4096, info=info)
    peak = torch.cuda.max_memory_allocated()
    assert info["tiles"] == 16 and out.shape == (H, W, 3)
    assert peak < 16 * 2 ** 30, f"peak device memory {peak / 2 ** 30:.1f} GiB"
    affine = info["affine"]
    r = sum(info["radius"])
    with torch.no_grad():
        # seams: a 2048 crop centred on the corner of four tiles, run whole-frame with the tiled run's affine map
        c0 = 8192 - 1024
        crop = content[c0:c0 + 2048, c0:c0 + 2048]
        z = net.forward_u8(torch.from_numpy(np.ascontiguousarray(crop)).cuda()[None])
        ref = net.inverse_u8(z.with_affines(affine[None]))[0].cpu().numpy()
        inner = slice(r, 2048 - r)
        d = np.abs(ref[inner, inner].astype(np.int16) - out[c0:c0 + 2048, c0:c0 + 2048][inner, inner].astype(np.int16))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, (d.max(), (d > 0).mean())
        # both image corners against the oracle: revnet_inverse(affine(revnet_forward(crop))) on 1024 crops, 512 corners
        torch.set_num_threads(16)
        T = affine[:1024].reshape(32, 32).double().cpu()
        t0 = affine[1024:].double().cpu()
        for which in ("tl", "br"):
            sl = slice(0, 1024) if which == "tl" else slice(H - 1024, H)
            x = torch.from_numpy(np.ascontiguousarray(content[sl, sl])).permute(2, 0, 1)[None].float().div(255.0)
            zo = cpu_ref.revnet_forward(x, sd, sp).double()
            zo = (torch.einsum("ij,bjhw->bihw", T, zo) + t0[None, :, None, None]).float()
            yo = cpu_ref.revnet_inverse(zo, sd, sp)[0].permute(1, 2, 0).mul(255.0).clamp(0, 255).byte().numpy()
            cs = slice(0, 512) if which == "tl" else slice(512, 1024)
            got = out[sl, sl][cs, cs].astype(np.int16)
            d = np.abs(got - yo[cs, cs].astype(np.int16))
            assert d.max() <= 1 and (d > 0).mean() < 1e-2, (which, d.max(), (d > 0).mean())
