"""Style maps on the GPU ("Style maps"): y = sum_k w_k(p) A_k(x) per code pixel, mixed inside the packed apply
kernels (cwct_apply_mix_pm_kernel, cwct_apply_pm128_kernel<BLEND, 2>) and by vst_cwct_mix_acc on dense codes.

The arithmetic is fixed (a_k as the plain apply computes it, m = w_0 a_0, m = m + w_k a_k, every operation rounded to fp32, no
FMA), so the main tests RESTATE it in eager torch from the plain routes' own results and ask for the same bits.  Shapes are
those of tests/test_gpu_strength.py: their 32-row tiles straddle the halves and the end of the code.  The weight maps are built
in row order (tests/style_map_ref.py: weight_rows) so that most tiles mix one-hot rows, multiples of 1/255 and arbitrary rows."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import test_gpu_parity as parity
from tests import test_gpu_strength as strength
from tests.zc import ptr, stream
from vstnet_amd import _lib
from vstnet_amd.synth import synthetic_frames

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cwct_ops_ref as O                                               # noqa: E402
import style_map_ref as R                                              # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
make_net, assert_close, NET_TOL, TOL = parity.make_net, parity.assert_close, parity.NET_TOL, parity.TOL
PHOTO, ART, code_hw, restate, make_map = strength.PHOTO, strength.ART, strength.code_hw, strength.restate, strength.make_map
PAD = 256


def make_weights(B, H, W, sp, K, seed):
    """[B,K,cH,cW] float32 on the device: style_map_ref.weight_rows (row order) scattered to image order"""
    cH, cW = code_hw(H, W, sp)
    perm = strength.row_pixels(H, W, sp)
    out = torch.empty(B, K, cH * cW, dtype=torch.float32, device="cuda")
    for b in range(B):
        out[b][:, perm] = T(R.weight_rows(cH * cW, K, seed + b)).cuda()
    return out.reshape(B, K, cH, cW)


def mix_restated(W, P):
    """w_0 P_0 + w_1 P_1 + ... in eager torch fp32, left to right: one rounding per operation, nothing fused"""
    m = W[:, 0:1] * P[0]
    for k in range(1, len(P)):
        m = m + W[:, k:k + 1] * P[k]
    return m


def style_frames(B, H, W, K):
    return [synthetic_frames(B, H + 4 * (k % 3), W + 4 * ((k + 1) % 2), seed=20 + k).cuda() for k in range(K)]


@pytest.fixture(scope="module")
def nets():
    out = {}
    for mode in ("photo", "art"):
        net, sd, sp = make_net(mode)
        net.packed_code = "always"
        out[mode] = (net, sd, sp)
    return out


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """a HIP error is sticky: nothing more is started on the card once a call has failed"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                            # noqa: BLE001
        pytest.exit(f"device error, stopping: {e}", returncode=3)


# ------------------------------------------------------------------------------------------------- 1. + 2. restated, one-hot
PACKED = [("photo", b, h, w, K) for b, h, w in PHOTO for K in (2, 3, 8)] + [("art", b, h, w, 2) for b, h, w in ART]


@pytest.mark.parametrize("mode,B,H,W,K", PACKED)
def test_packed_mix_restated_bit_for_bit(nets, mode, B, H, W, K):
    from models.cWCT import cWCT
    from vstnet_amd.code import PackedCode
    net, sd, sp = nets[mode]
    cw = cWCT()
    Wm = make_weights(B, H, W, sp, K, seed=31)
    s = make_map(B, H, W, sp, seed=11)
    with torch.no_grad():
        z = net(synthetic_frames(B, H, W, seed=5).cuda())
        zs = [net(f) for f in style_frames(B, H, W, K)]
        x = z.materialize()
        stats = [cw.style_stats(c) for c in zs]
        bound = cw.bind_style_map(Wm, z.shape, z.device)
        assert bound.K == K and bound.rows is not None
        for alpha_c in (0.0, 0.3):
            P = [cw.transfer_with_stats(z, st, alpha_c).materialize() for st in stats]
            want = mix_restated(Wm, P)
            for form, m in (("raw", Wm), ("bound", bound), ("3-D", Wm[0] if B == 1 else None)):
                if m is None:
                    continue
                t = cw.interpolation(z, zs, None, alpha_c, style_map=m)
                assert isinstance(t, PackedCode) and t.pending_mix is not None and tuple(t.pending_affines.shape[:2]) == (B, K)
                assert cw.last_style_map == "packed_rows" and cw.last_route == "packed_rows"
                assert torch.equal(t.materialize(), want), (form, alpha_c)
            t = cw.transfer_with_stats(z, stats, alpha_c, style_map=bound)
            assert cw.last_style_map == "packed_rows" and torch.equal(t.materialize(), want), alpha_c
            # a strength map on top: the mix first, then the existing blend
            t = cw.interpolation(z, zs, None, alpha_c, strength=s, style_map=bound)
            assert t.pending_strength is not None and cw.last_strength == "packed_rows"
            assert torch.equal(t.materialize(), restate(x, want, s)), alpha_c
            assert not torch.equal(P[0], P[1])                 # (there is something to mix)
        # a map that is one-hot k everywhere is the transfer of style k (alpha_c = 0.3, P from the loop's last turn)
        for k in range(K):
            hot = torch.zeros_like(Wm)
            hot[:, k] = 1.0
            t = cw.interpolation(z, zs, None, 0.3, style_map=hot)
            assert torch.equal(t.materialize(), P[k]), k
        cw.interpolation(z, zs, [1.0 / K] * K, 0.3)
        assert cw.last_style_map is None
        # refusals: weights next to a map, masks, a map bound for another code, a map of another K
        with pytest.raises(ValueError, match="alpha_s"):
            cw.interpolation(z, zs, [1.0 / K] * K, 0.3, style_map=bound)
        with pytest.raises(ValueError, match="style maps are not supported on the masked routes"):
            cw.interpolation(z, zs, None, 0.3, cmask=np.zeros((B,) + tuple(z.shape[2:]), np.uint8),
                             smask_list=[np.zeros((B,) + tuple(c.shape[2:]), np.uint8) for c in zs], style_map=bound)
        with pytest.raises(ValueError):
            cw.interpolation(zs[0], zs, None, 0.3, style_map=bound)
        with pytest.raises(ValueError, match="planes"):
            cw.interpolation(z, zs + zs[:1], None, 0.3, style_map=bound)


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2", "f16x2h"])
def test_decode_of_a_mixed_code(precision):
    """net(t, forward=False) and inverse_u8 (with and without luminance_of) mix while they load their state: the same bits as the
    decode of the materialised mixed code, packed from dense.  bf16x3: the state is the fp32 rows either way; the fp16 modes take
    the planes0 branch, whose split happens after the mix, on the fp32 values that presplit splits on the other side.  The plain
    transfer of one style goes the same way."""
    from models.cWCT import cWCT
    from vstnet_amd.code import from_dense
    cw = cWCT(precision=precision)
    for mode, shapes, K in (("photo", PHOTO, 3), ("art", ART, 2)):
        net, sd, sp = make_net(mode, precision)
        net.packed_code = "always"
        for B, H, W in shapes:
            x_img = synthetic_frames(B, H, W, seed=5).cuda()
            frames = (x_img.permute(0, 2, 3, 1) * 255).byte().contiguous()
            Wm = make_weights(B, H, W, sp, K, seed=37)
            s = make_map(B, H, W, sp, seed=17)
            with torch.no_grad():
                z = net(x_img)
                zs = [net(f) for f in style_frames(B, H, W, K)]
                pending = [cw.interpolation(z, zs, None, 0.3, style_map=Wm, **kw) for kw in ({}, {"strength": s})]
                for i, t in enumerate(pending + [cw.transfer(z, zs[0])]):
                    want = from_dense(t.materialize())
                    got, ref = net(t, forward=False), net(want, forward=False)
                    u8, u8_ref = net.inverse_u8(t), net.inverse_u8(want)
                    lum, lum_ref = net.inverse_u8(t, luminance_of=frames), net.inverse_u8(want, luminance_of=frames)
                    assert torch.equal(got, ref) and torch.equal(u8, u8_ref) and torch.equal(lum, lum_ref), (mode, B, H, W, i)


# ------------------------------------------------------------------------------------------------- 3. constant weights: oracle
def test_constant_weights_are_the_reference_interpolation(nets, golden):
    """W = (0.6, 0.4) everywhere, alpha_c = 0.3: the oracle's interpolation and the device's own, within parity.TOL"""
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    cw = cWCT()
    a_s, a_c = [0.6, 0.4], 0.3
    for mode, (B, H, W) in (("photo", (1, 48, 64)), ("art", (1, 48, 64))):
        net, sd, sp = nets[mode]
        with torch.no_grad():
            z, zs, zs2 = (net(synthetic_frames(B, H, W, seed=i).cuda()) for i in range(3))
            Wm = torch.tensor(a_s).reshape(1, 2, 1, 1).expand(B, 2, *z.shape[2:]).contiguous()
            t = cw.interpolation(z, [zs, zs2], None, a_c, style_map=Wm)
            assert cw.last_style_map == "packed_rows"
            ref = cpu_ref.interpolation(z.materialize().cpu(), [zs.materialize().cpu(), zs2.materialize().cpu()], a_s, a_c)
            assert_close(t.materialize(), ref, TOL, f"{mode}: constant map vs the oracle's interpolation")
            own = cw.interpolation(z, [zs, zs2], a_s, a_c)
            assert_close(t.materialize(), own.materialize(), TOL, f"{mode}: constant map vs the device's interpolation")
    # dense N = 8: the generic net of the goldens' architecture A
    g = golden("net_general")
    arch = ast.literal_eval(str(g["A_arch"]))
    sd = {k[len("A_w_"):]: T(g[k]) for k in g.files if k.startswith("A_w_")}
    net = RevResNet(**arch)
    net.load_state_dict(sd)
    net = net.to("cuda").eval()
    with torch.no_grad():
        z, zs, zs2 = net(T(g["A_x"]).cuda()), net(synthetic_frames(2, 20, 28, seed=9).cuda()), net(synthetic_frames(2, 24, 20, seed=8).cuda())
        assert z.shape[1] == 8
        Wm = torch.tensor(a_s).reshape(1, 2, 1, 1).expand(1, 2, *z.shape[2:]).contiguous()
        got = cw.interpolation(z, [zs, zs2], None, a_c, style_map=Wm)
        assert cw.last_style_map == "dense" and cw.last_route == "any_width_dense"
        assert_close(got, cpu_ref.interpolation(z.cpu(), [zs.cpu(), zs2.cpu()], a_s, a_c), TOL, "N = 8: constant map vs the oracle")
        assert_close(got, cw.interpolation(z, [zs, zs2], a_s, a_c), TOL, "N = 8: constant map vs the device's interpolation")


# ------------------------------------------------------------------------------------------------- 4. dense route
@pytest.mark.parametrize("N", [1, 8, 16, 100])
def test_mix_acc_entry_restated_bit_for_bit(N):
    """vst_cwct_mix_acc itself: scalar tail, pointers off the 16-byte grid (scalar form), out = a, first and later steps"""
    L = _lib.lib()
    rng = np.random.default_rng(N)
    for Lp in (2, 37, 4099):
        base = [T(rng.standard_normal(N * Lp + 1).astype(np.float32)).cuda() for _ in range(2)]
        w = T(rng.random(Lp, dtype=np.float32)).cuda()
        w[::3] = 1.0
        w[1::5] = 0.0
        for off in (0, 1):
            a, acc = base[0][off:off + N * Lp].reshape(N, Lp), base[1][off:off + N * Lp].reshape(N, Lp)
            for first, want in ((1, w[None] * a), (0, acc + w[None] * a)):
                out = acc.clone() if off == 0 else torch.cat([acc.new_zeros(1), acc.reshape(-1)])[1:].reshape(N, Lp)
                assert out.data_ptr() % 16 == (0 if off == 0 else 4)
                _lib.check(L.vst_cwct_mix_acc(ptr(a), ptr(w), ptr(out), N, Lp, first, stream()), "vst_cwct_mix_acc")
                assert torch.equal(out, want), (N, Lp, off, first)
            alias = base[0].clone()[off:off + N * Lp].reshape(N, Lp)        # out = a: first (w a in place) and later (a + w a)
            _lib.check(L.vst_cwct_mix_acc(ptr(alias), ptr(w), ptr(alias), N, Lp, 1, stream()), "vst_cwct_mix_acc")
            assert torch.equal(alias, w[None] * a), (N, Lp, off, "alias first")
            alias = base[0].clone()[off:off + N * Lp].reshape(N, Lp)
            _lib.check(L.vst_cwct_mix_acc(ptr(alias), ptr(w), ptr(alias), N, Lp, 0, stream()), "vst_cwct_mix_acc")
            assert torch.equal(alias, a + w[None] * a), (N, Lp, off, "alias later")


def test_dense_routes_restated_bit_for_bit(nets):
    """an artistic code with K = 3 (two sets of fragments fill the LDS: more styles go through the dense code), use_double at
    N = 32, and a plain dense N = 32 code with a strength map: from the K dense plain applies"""
    from models.cWCT import cWCT
    net, sd, sp = nets["art"]
    B, H, W, K = 1, 64, 96, 3
    with torch.no_grad():
        z = net(synthetic_frames(B, H, W, seed=5).cuda())
        zs = [net(f) for f in style_frames(B, H, W, K)]
        Wm = make_weights(B, H, W, sp, K, seed=41)
        cw = cWCT()
        stats = [cw.style_stats(c) for c in zs]
        P = [cw.transfer_with_stats(z.materialize(), st, 0.3) for st in stats]
        assert cw.last_route == "dense"
        got = cw.interpolation(z, zs, None, 0.3, style_map=Wm)
        assert cw.last_style_map == "dense" and cw.last_route == "dense" and not hasattr(got, "pending_mix")
        assert torch.equal(got, mix_restated(Wm, P))
        got = cw.transfer_with_stats(z, stats, 0.3, style_map=Wm)
        assert cw.last_style_map == "dense" and torch.equal(got, mix_restated(Wm, P))
        # use_double, N = 32
        net, sd, sp = nets["photo"]
        B, H, W, K = 2, 40, 24, 3
        z = net(synthetic_frames(B, H, W, seed=5).cuda())
        zs = [net(f) for f in style_frames(B, H, W, K)]
        Wm = make_weights(B, H, W, sp, K, seed=43)
        s = make_map(B, H, W, sp, seed=13)
        cw = cWCT(use_double=True)
        stats = [cw.style_stats(c) for c in zs]
        P = [cw.transfer_with_stats(z, st, 0.3) for st in stats]
        assert cw.last_route == "dense_f64"
        got = cw.interpolation(z, zs, None, 0.3, style_map=Wm)
        assert cw.last_style_map == "dense" and cw.last_route == "dense_f64" and torch.equal(got, mix_restated(Wm, P))
        # a plain tensor code, with a strength map on top (vst_cwct_blend after the sum)
        cw = cWCT()
        x = z.materialize().clone()
        zd = [c.materialize() for c in zs]                 # (dense styles on both sides: the same statistics kernel)
        P = [cw.transfer_with_stats(x, cw.style_stats(c), 0.0) for c in zd]
        got = cw.interpolation(x, zd, None, 0.0, strength=s, style_map=Wm)
        assert cw.last_style_map == "dense" and cw.last_strength == "dense"
        assert torch.equal(got, restate(x, mix_restated(Wm, P), s))


# ------------------------------------------------------------------------------------------------- 5. the kernel alone, fp64
class Guarded:
    """a float32 array of `n` elements behind and in front of PAD sentinel NaNs, 256-byte aligned"""

    def __init__(self, n, fill=None):
        self.n = int(n)
        self.buf = torch.full((PAD + self.n + PAD,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf[PAD:PAD + self.n]
        if fill is not None:
            self.view.copy_(T(np.ascontiguousarray(fill, dtype=np.float32).reshape(-1)))
        self.margins = self.buf.cpu().numpy().view(np.uint32).copy()

    def check(self):
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy().view(np.uint32)
        assert np.array_equal(now[:PAD], self.margins[:PAD]) and np.array_equal(now[-PAD:], self.margins[-PAD:]), "margin written"
        return self.view.cpu().numpy()


MIX_CODE_CASES = [(2, 12, 20, 2), (2, 24, 40, 3), (2, 24, 40, 8), (1, 24, 20, 2), (1, 48, 80, 2)]     # (sp, H, W, K)


@pytest.mark.parametrize("sp,H,W,K", MIX_CODE_CASES, ids=lambda v: str(v))
def test_apply_code_mix_against_fp64(sp, H, W, K):
    """vst_cwct_apply_code_mix on guarded views against the fp64 sum_k w_k (T_k x + t0_k), in the metric
    |err| / sum_k w_k (sum_j |T_k,ij| |x_j| + |t0_k,i|); bound FACTOR["apply"] x max(e32, U), e32 = the one-thread fp32
    restatement's error (tests/style_map_ref.py: mix32)."""
    N, rows = (32, H * W) if sp == 2 else (128, H * W // 4)
    x, affs, w = R.mix_input(N, K, rows, seed=sp + K)
    want, den = R.mix64(x, affs, w, N)
    e32 = O.apply_err(R.mix32(x, affs, w, N), want, den)
    code, aff, wr = Guarded(rows * N, x.T), Guarded(affs.size, affs), Guarded(w.size, w)
    out = Guarded(rows * N)
    rc = _lib.lib().vst_cwct_apply_code_mix(ptr(code.view), ptr(out.view), H, W, sp, ptr(aff.view), K, ptr(wr.view), None, stream())
    _lib.check(rc, "vst_cwct_apply_code_mix")
    got = out.check()
    for g, src in ((code, x.T), (aff, affs), (wr, w)):
        assert np.array_equal(g.check().view(np.uint32), np.ascontiguousarray(src, dtype=np.float32).reshape(-1).view(np.uint32))
    r = O.ratio("apply", O.apply_err(got.reshape(rows, N).T, want, den), e32)
    print(f"apply_code_mix sp={sp} {H}x{W} K={K}: e32 {e32 / O.U:.3g} u, device {r:.2f} x max(e32, floor), bound {O.FACTOR['apply']}")
    assert r <= O.FACTOR["apply"], (sp, H, W, K, r)
    # and with a strength map: the blend of the same sum (restated from the device's own mix, bit for bit)
    s = T(np.random.default_rng(K).random(rows, dtype=np.float32)).cuda()
    s[::4], s[1::7] = 1.0, 0.0
    outs = Guarded(rows * N)
    rc = _lib.lib().vst_cwct_apply_code_mix(ptr(code.view), ptr(outs.view), H, W, sp, ptr(aff.view), K, ptr(wr.view), ptr(s), stream())
    _lib.check(rc, "vst_cwct_apply_code_mix")
    xs, ms = T(np.ascontiguousarray(x.T)), T(got.reshape(rows, N))
    assert torch.equal(T(outs.check().reshape(rows, N)), restate(xs, ms, s.cpu()[:, None]))


# ------------------------------------------------------------------------------------------------- 6. scripts
# The decoder's receptive radius is 240 frame pixels (tiled.receptive_radius): a frame column equals a single-style run only
# where every code pixel within that radius has the one-hot weight.  The ramp therefore has plateaus: 0 up to column 256, 255
# from column 384 on, linear in between, on frames 640 wide; column 0 and the last column are then more than 240 pixels from any
# mixed code pixel and must equal the single-style runs exactly.
SW, SH = 640, 16


def _ramp(path):
    from PIL import Image
    xx = np.arange(SW)
    v = np.clip((xx - 256) * 255 // 128, 0, 255).astype(np.uint8)
    assert v[256] == 0 and v[257] > 0 and v[383] < 255 and v[384] == 255
    Image.fromarray(np.broadcast_to(v, (SH, SW)).copy()).save(path)
    return v


def _png_bytes(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


@pytest.mark.parametrize("mode", ["photorealistic", "artistic"])
def test_image_script_file_in_png_out(tmp_path, mode):
    from PIL import Image
    import image_transfer
    parity._png(tmp_path / "c.png", SH, SW, 40)
    parity._png(tmp_path / "s0.png", 40, 56, 6)
    parity._png(tmp_path / "s1.png", 36, 48, 7)
    ramp = _ramp(tmp_path / "m.png")
    base = ["--content", str(tmp_path / "c.png"), "--synthetic_weights", "--mode", mode]
    two = ["--styles", str(tmp_path / "s0.png"), str(tmp_path / "s1.png")]
    out = np.asarray(Image.open(image_transfer.main(base + two + ["--style_map", str(tmp_path / "m.png"), "--out_dir", str(tmp_path / "o")])))
    # the library call on the same inputs
    from models.cWCT import cWCT
    net = image_transfer.build_network(mode, None, True, torch.device("cuda"))
    cw = cWCT()
    imgs = [Image.open(tmp_path / f).convert("RGB") for f in ("c.png", "s0.png", "s1.png")]
    Wm = image_transfer.load_style_map([str(tmp_path / "m.png")], (SW, SH), mode)
    lib_out = image_transfer.stylize(net, cw, imgs[0], imgs[1:], style_map=Wm)
    assert cw.last_style_map == "packed_rows" and np.array_equal(out, lib_out)
    # the same two files as --style_maps (255 - v, v): the integer sum is 255 everywhere, so the same weights but for 1 - t
    # against (255 - v) / 255, one rounding apart: within one count
    Image.fromarray(np.broadcast_to(255 - ramp, (SH, SW)).copy()).save(tmp_path / "m0.png")
    out2 = np.asarray(Image.open(image_transfer.main(base + two + ["--style_maps", str(tmp_path / "m0.png"), str(tmp_path / "m.png"),
                                                                 "--out_dir", str(tmp_path / "o2")])))
    assert int(np.abs(out2.astype(int) - out.astype(int)).max()) <= 1
    singles = [np.asarray(Image.open(image_transfer.main(base + ["--style", str(tmp_path / f"s{k}.png"), "--out_dir",
                                                                 str(tmp_path / f"single{k}")]))) for k in range(2)]
    d0, d1 = (np.abs(out.astype(int) - s.astype(int)).max(axis=(0, 2)) for s in singles)
    print(f"{mode}: max |diff| to the first style over the 0 plateau {d0[:257].max()}, to the second over the 255 plateau "
          f"{d1[384:].max()}; column 0: {d0[0]}, last column: {d1[-1]}")
    assert d0[0] <= 1 and d1[-1] <= 1
    assert np.array_equal(out[:, 0], singles[0][:, 0]) and np.array_equal(out[:, -1], singles[1][:, -1])      # the ramp is 0 / 255
    assert not np.array_equal(singles[0], singles[1]) and d0[-1] > 0 and d1[0] > 0
    # with --alpha_c, --strength_map and --preserve_luminance on top: the library call again
    out3 = np.asarray(Image.open(image_transfer.main(base + two + ["--style_map", str(tmp_path / "m.png"), "--alpha_c", "0.3",
                                                                 "--strength_map", str(tmp_path / "m0.png"), "--preserve_luminance",
                                                                 "--out_dir", str(tmp_path / "o3")])))
    s = image_transfer.load_strength_map(str(tmp_path / "m0.png"), (SW, SH), mode)
    lib3 = image_transfer.stylize(net, cw, imgs[0], imgs[1:], alpha_c=0.3, preserve_luminance=True, strength=s, style_map=Wm)
    assert np.array_equal(out3, lib3) and not np.array_equal(out3, out)


def _clip_inputs(tmp_path, n):
    fd = tmp_path / "clip"
    fd.mkdir()
    for i in range(n):
        parity._png(fd / f"{i:03d}.png", SH, SW, 40 + i)
    parity._png(tmp_path / "s0.png", 40, 56, 6)
    parity._png(tmp_path / "s1.png", 36, 48, 7)
    _ramp(tmp_path / "m.png")
    return ["--video", str(fd), "--synthetic_weights", "--frames_only"], ["--styles", str(tmp_path / "s0.png"), str(tmp_path / "s1.png")]


def test_video_script_file_in_png_out(tmp_path):
    from PIL import Image
    import image_transfer
    import video_transfer
    base, two = _clip_inputs(tmp_path, 3)
    smap = ["--style_map", str(tmp_path / "m.png")]
    one = video_transfer.main(base + two + smap + ["--out_dir", str(tmp_path / "o")])
    got = _png_bytes(one)
    assert sorted(got) == ["%05d.png" % i for i in range(3)]
    # the library call, frame by frame: the styles bound and prefactored once, the map bound once
    from models.cWCT import cWCT
    from utils.utils import to_tensor_u8
    net = image_transfer.build_network("photorealistic", None, True, torch.device("cuda"))
    cw = cWCT()
    with torch.no_grad():
        stats = [cw.style_stats(net.forward_u8(to_tensor_u8(Image.open(tmp_path / f).convert("RGB")).cuda())) for f in ("s0.png", "s1.png")]
        bound = cw.bind_style_map(image_transfer.load_style_map([str(tmp_path / "m.png")], (SW, SH), "photorealistic"),
                                  (1, 32, SH, SW), "cuda")
        for i in range(3):
            z = net.forward_u8(to_tensor_u8(Image.open(tmp_path / "clip" / f"{i:03d}.png").convert("RGB")).cuda())
            want = net.inverse_u8(cw.transfer_with_stats(z, stats, 0.0, style_map=bound))[0].cpu().numpy()
            assert np.array_equal(np.asarray(Image.open(os.path.join(one, "%05d.png" % i))), want), i
    # the end columns against the single-style runs
    for k, col in ((0, 0), (1, -1)):
        single = video_transfer.main(base + ["--style", str(tmp_path / f"s{k}.png"), "--out_dir", str(tmp_path / f"single{k}")])
        for f in got:
            a, b = np.asarray(Image.open(os.path.join(one, f))), np.asarray(Image.open(os.path.join(single, f)))
            print(f"style {k} frame {f}: column {col} max |diff| {np.abs(a[:, col].astype(int) - b[:, col].astype(int)).max()}")
            assert np.array_equal(a[:, col], b[:, col]) and not np.array_equal(a, b), (k, f)
    # with the other flags it works with: the same frames from --resize device, and a run with --alpha_c, --strength_map and
    # --preserve_luminance differs and runs through
    assert _png_bytes(video_transfer.main(base + two + smap + ["--resize", "device", "--out_dir", str(tmp_path / "od")])) == got
    more = _png_bytes(video_transfer.main(base + two + smap + ["--alpha_c", "0.3", "--strength_map", str(tmp_path / "m.png"),
                                                               "--preserve_luminance", "--out_dir", str(tmp_path / "om")]))
    assert sorted(more) == sorted(got) and all(more[f] != got[f] for f in got)


def test_video_script_shards_and_gpus2_equal_one_process(tmp_path):
    import subprocess
    import video_transfer
    base, two = _clip_inputs(tmp_path, 5)
    args = base + two + ["--style_map", str(tmp_path / "m.png")]
    one = _png_bytes(video_transfer.main(args + ["--out_dir", str(tmp_path / "one")]))
    assert len(set(one.values())) == 5
    for r in range(2):
        two_dir = video_transfer.main(args + ["--out_dir", str(tmp_path / "two"), "--shard", f"{r}/2"])
    assert _png_bytes(two_dir) == one
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py")] + args + ["--out_dir", str(tmp_path / "g2"), "--gpus", "2"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _png_bytes(os.path.join(str(tmp_path / "g2"), os.path.basename(two_dir))) == one
