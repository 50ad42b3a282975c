"""Strength maps on the GPU: y = x + s (A(x) - x) per code pixel, blended inside the packed apply kernels
(cwct_apply_pm_kernel, cwct_apply_pm128_kernel, cwct_apply_labels_pm_kernel with BLEND) and by vst_cwct_blend on dense codes.

The arithmetic is fixed (every operation rounded to fp32, no FMA, s == 1 returns A(x)), so the main test RESTATES it in torch
from the parent's own routes and asks for the same bits.  Shapes are those of the packed tests of test_gpu_parity.py: their
32-row tiles straddle the halves and the end of the code."""
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import test_gpu_parity as parity
from tests.zc import ptr, stream
from vstnet_amd import _lib
from vstnet_amd.synth import synthetic_frames, synthetic_mask

pytestmark = pytest.mark.gpu
T = torch.from_numpy
make_net, assert_close, NET_TOL, TOL = parity.make_net, parity.assert_close, parity.NET_TOL, parity.TOL

PHOTO = [(1, 12, 20), (2, 40, 24), (1, 64, 96)]
ART = [(1, 12, 20), (1, 64, 96)]
MASKED = [(2, 40, 24, 4), (1, 96, 96, 8)]


def code_hw(H, W, sp):
    return (H, W) if sp == 2 else (H // 2, W // 2)


def row_pixels(H, W, sp):
    """pixel index (of the map at the code's resolution) of every packed row: vst_map_to_code on an index map"""
    cH, cW = code_hw(H, W, sp)
    idx = torch.arange(cH * cW, dtype=torch.float32, device="cuda")
    out = torch.empty_like(idx)
    _lib.check(_lib.lib().vst_map_to_code(ptr(idx), ptr(out), H, W, sp, stream()), "vst_map_to_code")
    return out.long()


def make_map(B, H, W, sp, seed):
    """[B,1,cH,cW] float32 on the device.  Built in ROW order, so that most 32-row tiles mix the four kinds of value (exact 0,
    exact 1, multiples of 1/255, arbitrary floats), then scattered to image order.  One run of consecutive rows is all 0 (it
    starts at row 8) and one is all 1 (it straddles the two halves): 256 rows each, or a quarter of the rows where the code
    has fewer than 784."""
    cH, cW = code_hw(H, W, sp)
    rows = cH * cW
    perm = row_pixels(H, W, sp)
    blk = 256 if rows >= 784 else rows // 4
    maps = []
    for b in range(B):
        rng = np.random.default_rng([seed, b])
        kind = rng.integers(0, 4, rows)
        v = rng.random(rows, dtype=np.float32)
        v = np.where(kind == 2, rng.integers(0, 256, rows).astype(np.float32) / np.float32(255), v)
        v = np.where(kind == 0, np.float32(0), np.where(kind == 1, np.float32(1), v)).astype(np.float32)
        v[8:8 + blk] = 0.0
        v[rows // 2 - blk // 2: rows // 2 - blk // 2 + blk] = 1.0
        img = torch.empty(rows, dtype=torch.float32, device="cuda")
        img[perm] = T(v).cuda()
        maps.append(img.reshape(1, cH, cW))
    return torch.stack(maps)


def restate(x, A, s):
    """the issue's arithmetic in torch fp32 (eager: one rounding per operation, nothing fused)"""
    return torch.where(s == 1, A, x + s * (A - x))


@pytest.fixture(scope="module")
def nets():
    out = {}
    for mode in ("photo", "art"):
        net, sd, sp = make_net(mode)
        net.packed_code = "always"
        out[mode] = (net, sd, sp)
    return out


# ------------------------------------------------------------------------------------------------------------ 1. row order
@pytest.mark.parametrize("H,W", [(12, 20), (40, 24), (64, 96)])
def test_map_rows_are_mask_rows(H, W):
    rng = np.random.default_rng(H)
    m = T(rng.integers(0, 200, (H, W), dtype=np.uint8)).cuda()
    mf = m.float().contiguous()
    rows_f, rows_u8 = torch.empty(H * W, dtype=torch.float32, device="cuda"), torch.empty(H * W, dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    _lib.check(L.vst_map_to_code(ptr(mf), ptr(rows_f), H, W, 2, stream()), "vst_map_to_code")
    _lib.check(L.vst_mask_to_code(ptr(m), ptr(rows_u8), H, W, stream()), "vst_mask_to_code")
    assert torch.equal(rows_f, rows_u8.float())


@pytest.mark.parametrize("sp,B,H,W", [(2, b, h, w) for b, h, w in PHOTO] + [(1, b, h, w) for b, h, w in ART])
def test_rows_round_trip_through_the_code(sp, B, H, W):
    """rows written into channel 0 of the packed rows come back as the map in channel 0 of the NCHW code (vst_code_to_z)"""
    from vstnet_amd.code import PackedCode
    cH, cW = code_hw(H, W, sp)
    N = 32 if sp == 2 else 128
    s = make_map(B, H, W, sp, seed=3)
    code = torch.zeros(B, cH * cW, N, device="cuda")
    L = _lib.lib()
    for b in range(B):
        rows = torch.empty(cH * cW, dtype=torch.float32, device="cuda")
        _lib.check(L.vst_map_to_code(ptr(s[b].contiguous()), ptr(rows), H, W, sp, stream()), "vst_map_to_code")
        code[b, :, 0] = rows
    z = PackedCode(code.reshape(B, -1), H, W, None, None, sp).materialize()
    assert tuple(z.shape) == (B, N, cH, cW)
    assert torch.equal(z[:, 0:1], s) and float(z[:, 1:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 2. restatement
@pytest.mark.parametrize("mode,B,H,W", [("photo", b, h, w) for b, h, w in PHOTO] + [("art", b, h, w) for b, h, w in ART])
def test_packed_blend_restated_bit_for_bit(nets, mode, B, H, W):
    from models.cWCT import cWCT
    from vstnet_amd.code import PackedCode
    net, sd, sp = nets[mode]
    cw = cWCT()
    x_img, xs, xs2 = (synthetic_frames(B, H, W, seed=5).cuda(), synthetic_frames(B, H + 8, W + 4, seed=6).cuda(),
                      synthetic_frames(B, H, W + 8, seed=7).cuda())
    s = make_map(B, H, W, sp, seed=11)
    with torch.no_grad():
        z, zs, zs2 = net(x_img), net(xs), net(xs2)
        x = z.materialize()
        stats = cw.style_stats(zs)
        bound = cw.bind_strength(s, z.shape, z.device)
        calls = {
            "transfer": lambda **k: cw.transfer(z, zs, **k),
            "interpolation": lambda **k: cw.interpolation(z, [zs, zs2], [0.6, 0.4], 0.3, **k),
            "transfer_with_stats": lambda **k: cw.transfer_with_stats(z, stats, 0.25, **k),
        }
        for name, call in calls.items():
            plain = call()
            A = plain.materialize()
            for form, st in (("raw", s), ("bound", bound), ("2-D", s[0, 0] if B == 1 else None)):
                if st is None:
                    continue
                t = call(strength=st)
                assert isinstance(t, PackedCode) and t.pending_strength is not None and cw.last_strength == "packed_rows"
                assert torch.equal(t.materialize(), restate(x, A, s)), (name, form)
            assert not torch.equal(A, x)                       # (there is something to blend)
            call()
            assert cw.last_strength is None
        # all ones: the transfer, all zeros: the code - rows and decoded frames, bit for bit
        plain = cw.transfer(z, zs)
        ones, zeros = cw.transfer(z, zs, strength=torch.ones_like(s)), cw.transfer(z, zs, strength=torch.zeros_like(s))
        assert torch.equal(ones.applied(), plain.applied()) and torch.equal(zeros.applied(), z.packed)
        assert torch.equal(net(ones, forward=False), net(plain, forward=False))
        assert torch.equal(net(zeros, forward=False), net(z, forward=False))
        assert torch.equal(net.inverse_u8(ones), net.inverse_u8(plain)) and torch.equal(net.inverse_u8(zeros), net.inverse_u8(z))
        # a bound map must fit the code
        with pytest.raises(ValueError):
            cw.transfer(zs, z, strength=bound)


@pytest.mark.parametrize("B,H,W,K", MASKED)
def test_masked_packed_blend_restated_bit_for_bit(nets, B, H, W, K):
    from models.cWCT import cWCT
    from vstnet_amd.code import PackedCode
    net, sd, sp = nets["photo"]
    cw = cWCT()
    x_img, xs = synthetic_frames(B, H, W, seed=2).cuda(), synthetic_frames(B, H, W, seed=3).cuda()
    cm = np.stack([synthetic_mask(H, W, K, seed=3 + b) for b in range(B)])                 # with a speck: label K has no slot
    sm = np.stack([synthetic_mask(H, W, K, seed=9 + b, speck=False) for b in range(B)])
    s = make_map(B, H, W, sp, seed=13)
    with torch.no_grad():
        z, zs = net(x_img), net(xs)
        x = z.materialize()
        plan = cw.learn_slots(cw.plan_masks(cm, sm, z.shape, zs.shape, z.device))
        assert 1 <= plan.max_slots <= 8
        for kw in ({}, {"alpha_s": [1.0], "alpha_c": 0.3}):
            plain = cw.transfer_with_plan(z, zs, plan, **kw)
            t = cw.transfer_with_plan(z, zs, plan, strength=s, **kw)
            assert isinstance(t, PackedCode) and t.pending_labels is not None and cw.last_strength == "packed_rows"
            assert cw.last_route.endswith("masked_packed_rows")
            A, got = plain.materialize(), t.materialize()
            assert torch.equal(got, restate(x, A, s)), kw
            speck = T(cm == K).cuda()[:, None].expand_as(x)
            assert int(speck.sum()) > 0 and torch.equal(got[speck], x[speck]), "rows without a slot keep the content rows"
        # the same through transfer(..., cmask, smask, strength=) on the dense code: masked_single_pass + vst_cwct_blend
        xd = x.clone()
        Ad = cw.transfer(xd, zs.materialize(), cm, sm)
        gd = cw.transfer(xd, zs.materialize(), cm, sm, strength=s)
        assert cw.last_route == "masked_single_pass" and cw.last_strength == "dense"
        assert torch.equal(gd, restate(xd, Ad, s)) and torch.equal(gd[speck], xd[speck])
        # in place: applied out of place, blended into the content code
        xi = x.clone()
        r = cw.transfer_with_plan(xi, zs.materialize(), cw.plan_masks(cm, sm, z.shape, zs.shape, z.device), inplace=True, strength=s)
        assert r.data_ptr() == xi.data_ptr() and torch.equal(r, gd)
        ones = cw.transfer_with_plan(z, zs, plan, strength=torch.ones_like(s))
        zeros = cw.transfer_with_plan(z, zs, plan, strength=torch.zeros_like(s))
        plain = cw.transfer_with_plan(z, zs, plan)
        assert torch.equal(ones.applied(), plain.applied()) and torch.equal(zeros.applied(), z.packed)
        assert torch.equal(net(ones, forward=False), net(plain, forward=False))
        assert torch.equal(net(zeros, forward=False), net(z, forward=False))


@pytest.mark.parametrize("N", [32, 128, 24])
def test_dense_blend_restated_bit_for_bit(N):
    """dense NCHW codes: the tuned widths and a width-generic one (N = 24), unmasked, per label, fp64, in place"""
    from models.cWCT import cWCT
    rng = np.random.default_rng(N)
    c = (T(rng.standard_normal((2, N, 24, 40)).astype(np.float32)) * 0.7 + 0.2).cuda()
    st = (T(rng.standard_normal((2, N, 20, 36)).astype(np.float32)) * 1.2 - 0.1).cuda()
    s = make_map(2, 24, 40, 2, seed=N)                      # (any map of the code's resolution; row order is of no concern here)
    cm, sm = np.stack([synthetic_mask(24, 40, 3, seed=1)] * 2), np.stack([synthetic_mask(20, 36, 3, seed=2, speck=False)] * 2)
    for cw in (cWCT(), cWCT(use_double=True)):
        A = cw.transfer(c, st)
        got = cw.transfer(c, st, strength=s)
        assert cw.last_strength == "dense" and ("any_width" in cw.last_route) == (N == 24)
        assert got.dtype == torch.float32 and torch.equal(got, restate(c, A, s)), cw.use_double
        Am = cw.transfer(c, st, cm, sm)
        gm = cw.transfer(c, st, cm, sm, strength=s)
        assert cw.last_strength == "dense" and torch.equal(gm, restate(c, Am, s)), (cw.last_route, cw.use_double)
        assert torch.equal(cw.transfer(c, st, strength=torch.ones_like(s)), A)
        assert torch.equal(cw.transfer(c, st, strength=torch.zeros_like(s)), c)
    cw = cWCT()
    stats = cw.style_stats(st)
    A = cw.transfer_with_stats(c, stats, 0.3)
    ci = c.clone()
    r = cw.transfer_with_stats(ci, stats, 0.3, inplace=True, strength=s)
    assert r.data_ptr() == ci.data_ptr() and torch.equal(r, restate(c, A, s))


def test_blend_entry_tail_alignment_and_aliasing():
    """vst_cwct_blend itself: N * L not a multiple of 4 (scalar tail), pointers off the 16-byte grid (scalar form), out = x, out = y"""
    L = _lib.lib()
    rng = np.random.default_rng(1)
    for N, Lp in ((7, 37), (3, 1021), (32, 64)):
        base = [T(rng.standard_normal(N * Lp + 1).astype(np.float32)).cuda() for _ in range(2)]
        sv = T(rng.random(Lp, dtype=np.float32)).cuda()
        sv[::3] = 1.0
        sv[1::5] = 0.0
        for off in (0, 1):
            x, y = base[0][off:off + N * Lp].reshape(N, Lp), base[1][off:off + N * Lp].reshape(N, Lp)
            want = restate(x, y, sv[None])
            out = torch.empty(N * Lp + 1, device="cuda")[off:off + N * Lp].reshape(N, Lp)
            _lib.check(L.vst_cwct_blend(ptr(x), ptr(y), ptr(sv), ptr(out), N, Lp, stream()), "vst_cwct_blend")
            assert torch.equal(out, want), (N, Lp, off)
            for alias in (0, 1):
                xa, ya = base[0].clone()[off:off + N * Lp].reshape(N, Lp), base[1].clone()[off:off + N * Lp].reshape(N, Lp)
                dst = (xa, ya)[alias]
                _lib.check(L.vst_cwct_blend(ptr(xa), ptr(ya), ptr(sv), ptr(dst), N, Lp, stream()), "vst_cwct_blend")
                assert torch.equal(dst, want), (N, Lp, off, alias)


# ------------------------------------------------------------------------------------------------------------ 3. decode
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2", "f16x2h"])
def test_decode_of_a_blended_code(precision):
    """net(t, forward=False) and inverse_u8 (with and without luminance_of) apply the pending map, and the blend, while they load
    their state: the same bits as the decode of the restated code, packed from dense.  The fp16 modes take the planes0 branch of
    the apply kernels, which rounds the fp32 values that presplit rounds on the other side, with the same split: equal, too.
    The plain transfer and the masked one go the same way, against their own materialised codes."""
    from models.cWCT import cWCT
    from vstnet_amd.code import from_dense
    cw = cWCT(precision=precision)

    def same_decode(net, t, dense, what, frames=None):
        want = from_dense(dense)
        assert torch.equal(net(t, forward=False), net(want, forward=False)), what
        assert torch.equal(net.inverse_u8(t), net.inverse_u8(want)), what
        if frames is not None:
            assert torch.equal(net.inverse_u8(t, luminance_of=frames), net.inverse_u8(want, luminance_of=frames)), what

    for mode, shapes in (("photo", PHOTO), ("art", ART)):
        net, sd, sp = make_net(mode, precision)
        net.packed_code = "always"
        for B, H, W in shapes:
            x_img, xs = synthetic_frames(B, H, W, seed=5).cuda(), synthetic_frames(B, H + 8, W + 4, seed=6).cuda()
            s = make_map(B, H, W, sp, seed=17)
            frames = (x_img.permute(0, 2, 3, 1) * 255).byte().contiguous()
            with torch.no_grad():
                z, zs = net(x_img), net(xs)
                plain = cw.transfer(z, zs)
                A = plain.materialize()
                same_decode(net, cw.transfer(z, zs, strength=s), restate(z.materialize(), A, s), (mode, B, H, W, "blend"), frames)
                same_decode(net, plain, A, (mode, B, H, W, "plain"), frames)
                # all ones / all zeros through the planes0 branch too
                assert torch.equal(net(cw.transfer(z, zs, strength=torch.ones_like(s)), forward=False), net(plain, forward=False))
                assert torch.equal(net(cw.transfer(z, zs, strength=torch.zeros_like(s)), forward=False), net(z, forward=False))
        if mode == "photo":
            B, H, W, K = MASKED[0]
            x_img, xs = synthetic_frames(B, H, W, seed=2).cuda(), synthetic_frames(B, H, W, seed=3).cuda()
            cm = np.stack([synthetic_mask(H, W, K, seed=3 + b) for b in range(B)])
            sm = np.stack([synthetic_mask(H, W, K, seed=9 + b, speck=False) for b in range(B)])
            s = make_map(B, H, W, sp, seed=19)
            with torch.no_grad():
                z, zs = net(x_img), net(xs)
                plan = cw.learn_slots(cw.plan_masks(cm, sm, z.shape, zs.shape, z.device))
                plain = cw.transfer_with_plan(z, zs, plan)
                A = plain.materialize()
                same_decode(net, cw.transfer_with_plan(z, zs, plan, strength=s), restate(z.materialize(), A, s), "masked blend")
                same_decode(net, plain, A, "masked plain")
                ones = cw.transfer_with_plan(z, zs, plan, strength=torch.ones_like(s))
                assert torch.equal(net(ones, forward=False), net(plain, forward=False))


# ------------------------------------------------------------------------------------------------------------ 4. oracle
def test_blend_vs_oracle(nets):
    """a constant map s = 1 - a IS the reference's alpha_c = a; a varying map against (1 - s) z_c + s transfer(z_c, z_s) in fp64.
    Tolerances: test_cwct_every_route_vs_oracle's for the same route, NET_TOL for decoded frames (a blend between x and A(x)
    adds at most three roundings to the error of A(x))."""
    from models.cWCT import cWCT
    from vstnet_amd.code import PackedCode
    rng = np.random.default_rng(5)
    cw = cWCT()
    a = 0.3
    # dense, N = 32
    c = T(rng.standard_normal((1, 32, 24, 40)).astype(np.float32)) * 0.7 + 0.2
    st = T(rng.standard_normal((1, 32, 20, 36)).astype(np.float32)) * 1.2 - 0.1
    const = torch.full((24, 40), 1.0 - a)
    assert_close(cw.transfer(c.cuda(), st.cuda(), strength=const), cpu_ref.interpolation(c, [st], [1.0], a), 2e-4,
                 "dense, constant map vs alpha_c", tol_max=TOL)
    s = make_map(1, 24, 40, 2, seed=23)
    sd64 = s.cpu().double()
    ref = (1 - sd64) * c.double() + sd64 * cpu_ref.transfer(c, st, use_double=True).double()
    assert_close(cw.transfer(c.cuda(), st.cuda(), strength=s), ref, 2e-4, "dense, varying map", tol_max=TOL)
    cm, sm = synthetic_mask(24, 40, 3, seed=1)[None], synthetic_mask(20, 36, 3, seed=2, speck=False)[None]
    ref = (1 - sd64) * c.double() + sd64 * cpu_ref.transfer_seg(c, st, cm, sm, use_double=True).double()
    assert_close(cw.transfer(c.cuda(), st.cuda(), cm, sm, strength=s), ref, 5e-4, "masked_single_pass, varying map", tol_max=5e-3)
    # packed rows from the network, code and decoded frame
    net, sd, sp = nets["photo"]
    xc, xs = synthetic_frames(1, 48, 64, seed=0), synthetic_frames(1, 48, 64, seed=1)
    s = make_map(1, 48, 64, 2, seed=29)
    sd64 = s.cpu().double()
    with torch.no_grad():
        z, zs = net(xc.cuda()), net(xs.cuda())
        zc, zsc = z.materialize().cpu(), zs.materialize().cpu()
        t = cw.transfer(z, zs, strength=torch.full((48, 64), 1.0 - a))
        assert isinstance(t, PackedCode) and cw.last_route == "packed_rows"
        assert_close(t.materialize(), cpu_ref.interpolation(zc, [zsc], [1.0], a), 2e-5, "packed_rows, constant map vs alpha_c")
        t = cw.transfer(z, zs, strength=s)
        ref = (1 - sd64) * zc.double() + sd64 * cpu_ref.transfer(zc, zsc, use_double=True).double()
        assert_close(t.materialize(), ref, 2e-5, "packed_rows, varying map")
        assert_close(net(t, forward=False), cpu_ref.revnet_inverse(ref.float(), sd, sp), NET_TOL["bf16x3"], "decoded frame, varying map")
        cm2, sm2 = synthetic_mask(48, 64, 3, seed=3)[None], synthetic_mask(48, 64, 3, seed=4, speck=False)[None]
        plan = cw.learn_slots(cw.plan_masks(cm2, sm2, z.shape, zs.shape, z.device))
        tm = cw.transfer_with_plan(z, zs, plan, strength=s)
        assert isinstance(tm, PackedCode) and cw.last_route == "masked_packed_rows"
        ref = (1 - sd64) * zc.double() + sd64 * cpu_ref.transfer_seg(zc, zsc, cm2, sm2, use_double=True).double()
        assert_close(tm.materialize(), ref, 2e-4, "masked_packed_rows, varying map", tol_max=TOL)
    # artistic rows
    net, sd, sp = nets["art"]
    xc, xs = synthetic_frames(1, 64, 64, seed=0), synthetic_frames(1, 64, 64, seed=1)
    s = make_map(1, 64, 64, 1, seed=31)
    sd64 = s.cpu().double()
    with torch.no_grad():
        z, zs = net(xc.cuda()), net(xs.cuda())
        zc, zsc = z.materialize().cpu(), zs.materialize().cpu()
        t = cw.transfer(z, zs, strength=s)
        ref = ((1 - sd64) * zc.double() + sd64 * cpu_ref.transfer(zc, zsc).double()).float()
        assert_close(net(t, forward=False), cpu_ref.revnet_inverse(ref, sd, sp), NET_TOL["bf16x3"], "artistic decoded frame, varying map")


# ------------------------------------------------------------------------------------------------------------ 5. pipeline, scripts
def test_frame_pipeline_with_a_bound_map(nets):
    """three streams share one bound map: the frames of the sequential loop, bit for bit"""
    from models.cWCT import cWCT
    from vstnet_amd.pipeline import FramePipeline, AsyncSink, prefetch
    net, sd, sp = nets["photo"]
    cw = cWCT()
    H, W, n = 64, 96, 8
    frames = [(synthetic_frames(1, H, W, seed=100 + i)[0].permute(1, 2, 0) * 255).byte().numpy() for i in range(n)]
    style = (synthetic_frames(1, 48, 64, seed=7)[0].permute(1, 2, 0) * 255).byte()[None].cuda()
    cmask, smask = synthetic_mask(H, W, 3, seed=1)[None], synthetic_mask(48, 64, 3, seed=2)[None]
    with torch.no_grad():
        z_s = net.forward_u8(style)
        stats = cw.style_stats(z_s)
        bound = cw.bind_strength(make_map(1, H, W, 2, seed=37), (1, 32, H, W), "cuda")
        plan = cw.bind_style(cw.learn_slots(cw.plan_masks(cmask, smask, (1, 32, H, W), z_s.shape, z_s.device)), z_s)
        for masked in (False, True):
            tf = ((lambda z, i: cw.transfer_with_plan(z, None, plan, strength=bound)) if masked
                  else (lambda z, i: cw.transfer_with_stats(z, stats, strength=bound)))
            ref = [net.inverse_u8(tf(net.forward_u8(T(f)[None].cuda()), i))[0].cpu().numpy() for i, f in enumerate(frames)]
            plain = net.inverse_u8(cw.transfer_with_stats(net.forward_u8(T(frames[0])[None].cuda()), stats))[0].cpu().numpy()
            assert masked or not np.array_equal(ref[0], plain), "the map changes the frame"
            got = {}
            sink = AsyncSink(lambda i, arr: got.__setitem__(i, arr))
            pipe = FramePipeline(net, tf, H, W, depth=4, compute_streams=3)
            assert pipe.run(prefetch(iter(frames), ahead=2), sink) == n
            sink.close()
            for i in range(n):
                assert np.array_equal(got[i], ref[i]), (masked, i)


def _png(path, h, w, seed):
    return parity._png(path, h, w, seed)


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("masked", [False, True])
def test_video_script_with_a_strength_map(tmp_path, masked):
    """5 frames of 48 x 64 and a gradient map: two shards write the PNG bytes of one process, the map changes the frames, and an
    all-white map is the run without the flag, byte for byte."""
    from PIL import Image
    import video_transfer
    fd = tmp_path / "clip"
    fd.mkdir()
    for i in range(5):
        _png(fd / f"{i:03d}.png", 48, 64, 40 + i)
    _png(tmp_path / "s.png", 40, 56, 6)
    yy, xx = np.mgrid[0:24, 0:32]
    Image.fromarray(((xx * 255) // 31).astype(np.uint8)).save(tmp_path / "grad.png")       # resized (BILINEAR) to 64 x 48
    Image.fromarray(np.full((48, 64), 255, np.uint8)).save(tmp_path / "white.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only"]
    if masked:
        md = tmp_path / "maps"
        md.mkdir()
        for i in range(5):
            Image.fromarray(synthetic_mask(48, 64, 3, seed=50 + i, speck=False)).save(md / f"{i:03d}.png")
        Image.fromarray(synthetic_mask(40, 56, 3, seed=2, speck=False)).save(tmp_path / "sseg.png")
        base += ["--content_seg_dir", str(md), "--style_seg", str(tmp_path / "sseg.png")]
    run = lambda out, *extra: video_transfer.main(base + ["--out_dir", str(tmp_path / out)] + list(extra))      # noqa: E731
    one = _files(run("one", "--strength_map", str(tmp_path / "grad.png")))
    for r in range(2):
        two_dir = run("two", "--strength_map", str(tmp_path / "grad.png"), "--shard", f"{r}/2")
    none = _files(run("none"))
    white = _files(run("white", "--strength_map", str(tmp_path / "white.png")))
    assert sorted(one) == ["%05d.png" % i for i in range(5)]
    assert _files(two_dir) == one
    assert white == none
    assert all(one[f] != none[f] for f in one)


def test_video_script_redo_past_eight_labels_with_a_strength_map(tmp_path):
    """Per-frame maps with 16 valid labels: every frame overflows the packed route's 8 slots and is done again on the dense
    route (transfer_with_plan on the PackedCode with a 32-slot plan: vst_cwct_apply_labels, then vst_cwct_blend).  The frames
    are the library's, byte for byte, and the dense masked blend on a PackedCode is the restated arithmetic, bit for bit."""
    from PIL import Image
    import video_transfer
    from models.cWCT import cWCT
    from vstnet_amd.code import PackedCode
    from utils.utils import to_tensor_u8
    H, W, n = 96, 128, 3
    fd, md = tmp_path / "clip", tmp_path / "maps"
    fd.mkdir()
    md.mkdir()
    frames = [_png(fd / f"{i:03d}.png", H, W, 60 + i) for i in range(n)]
    style = _png(tmp_path / "s.png", H, W, 9)
    bands = np.repeat(np.arange(16, dtype=np.uint8), 8)[None].repeat(H, 0)         # 16 labels of 8 x 96 pixels each
    masks = [np.roll(bands, 8 * i, axis=1) for i in range(n)]
    for i, m in enumerate(masks):
        Image.fromarray(m).save(md / f"{i:03d}.png")
    Image.fromarray(bands).save(tmp_path / "sseg.png")
    yy, xx = np.mgrid[0:H, 0:W]
    grad = ((xx * 255) // (W - 1)).astype(np.uint8)
    grad[: H // 4] = 0
    grad[-(H // 4):] = 255
    Image.fromarray(grad).save(tmp_path / "grad.png")
    out = video_transfer.main(["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only",
                               "--content_seg_dir", str(md), "--style_seg", str(tmp_path / "sseg.png"),
                               "--out_dir", str(tmp_path / "o"), "--strength_map", str(tmp_path / "grad.png")])
    assert video_transfer.LAST_RUN["redo"] == n, "every frame takes the dense route"
    net, sd, sp = make_net("photo")
    cw = cWCT()
    s = T(grad.astype(np.float32) / np.float32(255)).cuda()
    with torch.no_grad():
        binding = cw.bind_style_labels(net.forward_u8(to_tensor_u8(Image.fromarray(style)).cuda()), bands[None])
        for i in range(n):
            z = net.forward_u8(to_tensor_u8(Image.fromarray(frames[i])).cuda())
            plan = lambda: cw.plan_frame(T(masks[i]).cuda(), binding, max_slots=32)      # noqa: E731
            A = cw.transfer_with_plan(z, None, plan())
            t = cw.transfer_with_plan(z, None, plan(), strength=s)
            assert not isinstance(t, PackedCode) and cw.last_route == "masked_single_pass" and cw.last_strength == "dense"
            assert not torch.equal(A, z.materialize())
            assert torch.equal(t, restate(z.materialize(), A, s[None, None])), i
            got = np.asarray(Image.open(os.path.join(out, "%05d.png" % i)))
            assert np.array_equal(got, net.inverse_u8(t)[0].cpu().numpy()), i


def test_image_script_with_a_strength_map(tmp_path):
    """image_transfer.py --strength_map writes the bytes of the library call on the same pixels and map"""
    from PIL import Image
    import image_transfer
    from models.cWCT import cWCT
    from utils.utils import to_tensor_u8
    c = _png(tmp_path / "c.png", 48, 64, 1)
    s = _png(tmp_path / "s.png", 40, 40, 2)
    yy, xx = np.mgrid[0:30, 0:50]
    Image.fromarray(((yy * 255) // 29).astype(np.uint8)).save(tmp_path / "m.png")
    for mode in ("photorealistic", "artistic"):
        out = image_transfer.main(["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--mode", mode,
                                   "--out_dir", str(tmp_path / ("o_" + mode)), "--synthetic_weights",
                                   "--strength_map", str(tmp_path / "m.png")])
        got = np.asarray(Image.open(out))
        net, sd, sp = make_net("photo" if mode == "photorealistic" else "art")
        cw = cWCT()
        m = image_transfer.load_strength_map(str(tmp_path / "m.png"), (64, 48), mode)
        assert m.shape == ((48, 64) if sp == 2 else (24, 32))
        with torch.no_grad():
            z, zs = net.forward_u8(to_tensor_u8(Image.fromarray(c)).cuda()), net.forward_u8(to_tensor_u8(Image.fromarray(s)).cuda())
            want = net.inverse_u8(cw.transfer(z, zs, strength=m))[0].cpu().numpy()
            plain = net.inverse_u8(cw.transfer(z, zs))[0].cpu().numpy()
        assert np.array_equal(got, want) and not np.array_equal(got, plain), mode
