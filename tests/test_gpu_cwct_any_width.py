"""GPU: the width-generic cWCT (csrc/cwct_any.hip) — codes of any width N = 1..256 outside the tuned {16, 32, 64, 128} stylise
like the reference (oracle/cpu_ref.py), with the route they take asserted."""
import ast

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests.zc import rel_err

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def assert_close(got, ref, tol, what, tol_max=None):
    l2, mx = rel_err(got, ref)
    tol_max = tol if tol_max is None else tol_max
    assert l2 <= tol and mx <= tol_max, f"{what}: rel-L2 {l2:.3e}, max-rel {mx:.3e} (tol {tol:g}/{tol_max:g})"
    return l2, mx


def code(B, N, H, W, seed, mean=3.0):
    """a correlated, well-conditioned code (the mixing matrix's eigenvalues lie within 0.5 of 1) with a large mean (the
    statistics must not cancel)"""
    g = torch.Generator().manual_seed(seed)
    mix = 0.5 * torch.randn(N, N, generator=g) / np.sqrt(N) + torch.eye(N)
    x = mix @ torch.randn(B, N, H * W, generator=g) + mean + torch.randn(B, N, 1, generator=g)
    return x.reshape(B, N, H, W).float().contiguous()


def sizes(N):
    """ragged content / style sizes with L >= 4 N"""
    return ((24, 40), (17, 23)) if 4 * N <= 17 * 23 else ((40, 56), (37, 41))


def masks(B, H, W, seed, tiny):
    """3 labels: 0 (left), 1 (right), 2 (a speck of `tiny` pixels: invalid by the count rule in the content map)"""
    out = []
    for b in range(B):
        m = np.zeros((H, W), np.uint8)
        m[:, W // 2 + b:] = 1
        if tiny:
            m.reshape(-1)[seed + b: seed + b + tiny] = 2
        out.append(m)
    return out


@pytest.mark.parametrize("N", [1, 2, 3, 8, 12, 24, 48, 96, 100, 160, 256])
def test_transfer_any_width_vs_oracle(N):
    from models.cWCT import cWCT
    (cH, cW), (sH, sW) = sizes(N)
    for B in (1, 2):
        c, s = code(B, N, cH, cW, seed=N * 10 + B), code(B, N, sH, sW, seed=N * 10 + B + 5)
        cw = cWCT()
        got = cw.transfer(c.cuda(), s.cuda())
        assert cw.last_route == "any_width_dense"
        assert_close(got, cpu_ref.transfer(c, s), 2e-4, f"transfer N={N} B={B}", tol_max=1e-3)


@pytest.mark.parametrize("N", [8, 48])
def test_interpolation_two_styles(N):
    from models.cWCT import cWCT
    c, s1, s2 = code(2, N, 24, 40, 1), code(2, N, 17, 23, 2, mean=-1.0), code(2, N, 20, 20, 3, mean=0.5)
    cw = cWCT()
    for ac in (0.0, 0.3):
        got = cw.interpolation(c.cuda(), [s1.cuda(), s2.cuda()], [0.6, 0.4], ac)
        assert cw.last_route == "any_width_dense"
        assert_close(got, cpu_ref.interpolation(c, [s1, s2], [0.6, 0.4], ac), 2e-4, f"interp N={N} ac={ac}", tol_max=1e-3)


@pytest.mark.parametrize("N", [8, 48])
def test_masked_transfer_per_label(N):
    from models.cWCT import cWCT
    c, s = code(2, N, 32, 48, 11), code(2, N, 30, 34, 12, mean=-2.0)
    cm, sm = masks(2, 32, 48, 5, tiny=6), masks(2, 30, 34, 7, tiny=40)
    for b in range(2):
        labels, ok = cpu_ref.compute_label_info(cm[b], sm[b])
        assert list(labels) == [0, 1, 2] and list(ok[:3]) == [1, 1, 0]
    cw = cWCT()
    got = cw.transfer(c.cuda(), s.cuda(), cm, sm)
    assert cw.last_route == "any_width_masked_per_label"
    assert_close(got, cpu_ref.transfer_seg(c, s, cm, sm), 1e-4, f"transfer_seg N={N}", tol_max=1e-3)
    for b in range(2):
        keep = T(cm[b].reshape(-1) == 2)
        assert torch.equal(got[b].reshape(N, -1)[:, keep].cpu(), c[b].reshape(N, -1)[:, keep])


@pytest.mark.parametrize("N", [8, 48])
def test_use_double_any_width(N):
    from models.cWCT import cWCT
    c, s = code(2, N, 32, 48, 21), code(2, N, 30, 34, 22, mean=-2.0)
    cw = cWCT(use_double=True)
    got = cw.transfer(c.cuda(), s.cuda())
    assert cw.last_route == "any_width_dense_f64"
    assert_close(got, cpu_ref.transfer(c, s, use_double=True), 2e-6, f"fp64 transfer N={N}")
    cm, sm = masks(2, 32, 48, 5, tiny=6), masks(2, 30, 34, 7, tiny=40)
    got = cw.transfer(c.cuda(), s.cuda(), cm, sm)
    assert cw.last_route == "any_width_masked_per_label_f64"
    assert_close(got, cpu_ref.transfer_seg(c, s, cm, sm, use_double=True), 2e-6, f"fp64 transfer_seg N={N}")


def test_jitter_at_native_sizes(golden):
    from models.cWCT import cWCT
    g = golden("cwct_jitter")
    cw = cWCT()
    L1 = cw.cholesky_dec(T(g["neg_in"]).cuda())                # diag(1, -3e-5): two retries
    assert int(cw.last_info[2]) == int(g["neg_tries"]) == 2
    assert_close(L1, T(g["neg_L"]), 1e-5, "chol diag(1,-3e-5)")
    L2 = cw.cholesky_dec(torch.ones(4, 4).cuda())              # exactly singular: one retry
    assert int(cw.last_info[2]) == int(g["ones4_tries"]) == 1
    assert_close(L2, T(g["ones4_L"]), 1e-3, "chol ones(4,4)")
    # rank-deficient code: 48 channels, 6 x 6 pixels
    x = code(1, 48, 6, 6, 31, mean=0.0)
    xc = x.reshape(48, -1) - x.reshape(48, -1).mean(-1, keepdim=True)
    conv = (xc @ xc.t()) / (xc.shape[1] - 1)
    L_ref, tries = cpu_ref.cholesky_dec(conv, return_tries=True)
    assert tries >= 1
    L3 = cw.cholesky_dec(conv.cuda())
    assert int(cw.last_info[2]) == tries
    assert_close(L3 @ L3.t(), L_ref @ L_ref.t(), 1e-4, "jittered L L^T (N = 48)")
    cw.transfer(x.cuda(), code(1, 48, 16, 16, 32).cuda())
    assert int(cw.last_info[0]) == tries                         # the content side of the transfer jitters the same way
    # B = 2, only sample 0 singular (a constant channel): the reference's batched Cholesky jitters both samples
    c = code(2, 8, 24, 40, 41) * 0.05
    c[0, 3] = 1.0
    s = code(2, 8, 17, 23, 42)
    got = cw.transfer(c.cuda(), s.cuda())
    assert int(cw.last_info[0]) >= 1
    ref = cpu_ref.transfer(c, s)
    assert_close(got[1], ref[1], 2e-5, "coupled sample", tol_max=1e-4)
    alone = cpu_ref.transfer(c[1:2], s[1:2])
    assert rel_err(alone[0], ref[1])[0] > 1e-5                   # (the coupling is what the comparison pins)


@pytest.mark.parametrize("N", [8, 100])
def test_cached_style_equals_transfer(N):
    from models.cWCT import cWCT
    (cH, cW), (sH, sW) = sizes(N)
    c, s = code(2, N, cH, cW, 51).cuda(), code(2, N, sH, sW, 52).cuda()
    cw = cWCT()
    ref = cw.transfer(c, s)
    ss = cw.style_stats(s)
    assert all(float(t[0]) < 0 for t in ss)                       # prefactored records
    got = cw.transfer_with_stats(c, ss)
    assert cw.last_route == "any_width_dense"
    assert_close(got, ref, 1e-6, f"transfer_with_stats N={N}")
    cc = c.clone()
    out = cw.transfer_with_stats(cc, ss, inplace=True)
    assert out.data_ptr() == cc.data_ptr()
    assert_close(cc, ref, 1e-6, f"transfer_with_stats in place N={N}")


@pytest.mark.parametrize("N", [32, 128])
def test_width_generic_kernels_agree_with_tuned(N, monkeypatch):
    """the _n entry points at widths that also have tuned kernels (precision fp32)"""
    import vstnet_amd.cwct as cwct_mod
    from models.cWCT import cWCT
    c, s = code(2, N, 40, 56, 61).cuda(), code(2, N, 37, 41, 62).cuda()
    tuned = cWCT(precision="fp32")
    ref = tuned.transfer(c, s)
    ref_stats = tuned.stats(c[0].reshape(N, -1))
    assert tuned.last_route == "dense"
    monkeypatch.setattr(cwct_mod, "_SUPPORTED_N", ())
    generic = cWCT(precision="fp32")
    got = generic.transfer(c, s)
    assert generic.last_route == "any_width_dense"
    assert_close(generic.stats(c[0].reshape(N, -1)), ref_stats, 1e-6, f"stats_n vs stats N={N}")
    assert_close(got, ref, 1e-5, f"_n vs tuned N={N}", tol_max=1e-4)


def test_golden_arch_a_end_to_end(golden):
    """RevResNet(hidden_dim=4) -> an 8-channel code: forward, cWCT, inverse on the GPU against the oracle"""
    from models.RevResNet import RevResNet
    from models.cWCT import cWCT
    from vstnet_amd.synth import synthetic_frames
    g = golden("net_general")
    arch = ast.literal_eval(str(g["A_arch"]))
    sd = {k[len("A_w_"):]: T(g[k]) for k in g.files if k.startswith("A_w_")}
    net = RevResNet(**arch)
    net.load_state_dict(sd)
    net = net.to("cuda").eval()
    xc, xs = T(g["A_x"]), synthetic_frames(2, 20, 28, seed=9)
    with torch.no_grad():
        zc, zs = cpu_ref.revnet_forward(xc, sd, arch["sp_steps"], arch), cpu_ref.revnet_forward(xs, sd, arch["sp_steps"], arch)
        assert zc.shape[1] == 8
        ref = cpu_ref.revnet_inverse(cpu_ref.transfer(zc, zs), sd, arch["sp_steps"], 3, arch)
        cw = cWCT()
        got = net(cw.transfer(net(xc.cuda()), net(xs.cuda())), forward=False)
        assert cw.last_route == "any_width_dense"
        assert_close(got, ref, 5e-5, "arch A stylised frame vs oracle")
        cm, sm = masks(2, 16, 24, 3, tiny=5), masks(2, 20, 28, 4, tiny=0)
        ref = cpu_ref.revnet_inverse(cpu_ref.transfer_seg(zc, zs, cm, sm), sd, arch["sp_steps"], 3, arch)
        got = net(cw.transfer(net(xc.cuda()), net(xs.cuda()), cm, sm), forward=False)
        assert cw.last_route == "any_width_masked_per_label"
        assert_close(got, ref, 5e-5, "arch A masked stylised frame vs oracle")
