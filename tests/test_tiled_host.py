"""CPU: the host side of the halo-tiled stylisation (vstnet_amd/tiled.py) - receptive radii, tile plans, the statistics merge
and the C ABI of the rectangle statistics and the whole-frame guard.  No compute call reaches the GPU: every C call here fails
its argument or shape check before it would touch memory."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from vstnet_amd import _lib, tiled

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null pointer that no call below may dereference


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _net(mode):
    from models.RevResNet import RevResNet
    return RevResNet(hidden_dim=16, sp_steps=2) if mode == "photo" else RevResNet(hidden_dim=64, sp_steps=1)


@pytest.mark.parametrize("mode,r_f,r_i", [("photo", 232, 240), ("art", 232, 236)])
def test_receptive_radius_matches_the_hand_derivation(mode, r_f, r_i):
    """DESIGN.md "Ultra-resolution" derives these by hand: forward 1*27 + 2*30 + 4*36 (block 0 sees a zero half) plus the
    alignment of the two stride-2 blocks and the quarter-resolution cell; inverse 1*30 + 2*30 + 4*36 plus alignment."""
    net = _net(mode)
    assert tiled.receptive_radius(net, "forward") == r_f
    assert tiled.receptive_radius(net, "inverse") == r_i
    assert r_f % 4 == 0 and r_i % 4 == 0
    with pytest.raises(ValueError):
        tiled.receptive_radius(net, "sideways")


def test_receptive_radius_generic_architecture_is_not_supported():
    from models.RevResNet import RevResNet
    net = RevResNet(nBlocks=[2, 2, 2], hidden_dim=16, sp_steps=2)
    with pytest.raises(NotImplementedError, match="published architectures"):
        tiled.receptive_radius(net, "forward")


def test_cone_is_exact_for_a_single_block():
    """One stride-1 block with 3x3 convs reaches 3 pixels, a stride-2 one 3 + alignment at half resolution."""
    assert tiled._residual((10, 10), 1, 3) == (7, 13)
    assert tiled._conv((10, 10), 2, 1) == (5, 5)
    assert tiled._conv((11, 11), 2, 1) == (5, 6)


@pytest.mark.parametrize("H,W,tile", [(16384, 16384, 4096), (8192, 4100, 2048), (1028, 2052, 512), (64, 96, 1024),
                                      (4100, 8, 1000), (3072, 2048, 1024)])
def test_tile_plan_partitions_the_frame(H, W, tile):
    halo = 472
    limit = 1 << 26
    tiles = tiled.tile_plan(H, W, tile, halo, limit)
    ys = sorted({(t.iy0, t.iy1) for t in tiles})
    xs = sorted({(t.ix0, t.ix1) for t in tiles})
    assert len(tiles) == len(ys) * len(xs)               # a grid
    for edges, n in ((ys, H), (xs, W)):                  # each axis: consecutive intervals that cover [0, n) exactly once
        assert edges[0][0] == 0 and edges[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(edges[:-1], edges[1:]))
        assert all(8 <= b - a <= max(tile, 8) + 3 for a, b in edges)
    if H * W <= 1 << 22:                                 # and in 2-D, where the count array is small
        cover = np.zeros((H, W), np.int32)
        for t in tiles:
            cover[t.iy0:t.iy1, t.ix0:t.ix1] += 1
        assert (cover == 1).all()
    for t in tiles:
        assert all(v % 4 == 0 for v in t)
        assert t.wy0 == max(0, t.iy0 - halo) and t.wy1 == min(H, t.iy1 + halo)   # grown by the halo, clipped at the border
        assert t.wx0 == max(0, t.ix0 - halo) and t.wx1 == min(W, t.ix1 + halo)
        h, w = t.window_hw
        assert h >= 8 and w >= 8 and h * w <= limit
        y0, x0, ih, iw = t.rect
        assert 0 <= y0 and y0 + ih <= h and 0 <= x0 and x0 + iw <= w
    if tile >= max(H, W):
        assert tiles == [tiled.Tile(0, H, 0, W, 0, H, 0, W)]


def test_tile_plan_refuses_windows_past_the_guard():
    with pytest.raises(ValueError, match="smaller tile"):
        tiled.tile_plan(16384, 16384, 8192, 472, 1 << 26)
    with pytest.raises(ValueError):
        tiled.tile_plan(1026, 1024, 512, 472)


def test_default_tile_and_the_tiling_decision():
    t = tiled.default_tile(472, 1 << 40, 1 << 26)
    assert t % 512 == 0 and (t + 944) ** 2 <= 1 << 26 and (t + 512 + 944) ** 2 > 1 << 26
    small = tiled.default_tile(472, 4 << 30, 1 << 26)
    assert small < t and (small + 944) ** 2 * tiled.WINDOW_BYTES_PER_PX <= 4 << 30
    assert tiled.needs_tiling(16384, 16384, 1 << 40, 1 << 26)
    assert not tiled.needs_tiling(8192, 8192, 1 << 40, 1 << 26)
    assert tiled.needs_tiling(8192, 8192, 1 << 30, 1 << 26)       # past the memory budget
    assert not tiled.needs_tiling(1024, 1024, 4 << 30, 1 << 26)


def _record(x):
    """{n, mean, cov} of the columns of x [N, L] in float64 (cov 0/0 for L = 1, as the kernels give it)."""
    N, L = x.shape
    mean = x.mean(1) if L else np.zeros(N)
    d = x - mean[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = d @ d.T / (L - 1)
    return torch.from_numpy(np.concatenate([[float(L)], mean, cov.reshape(-1)]))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_merge_stats_of_random_partitions(seed):
    rng = np.random.default_rng(seed)
    N, L = 32, 5000
    x = rng.normal(size=(N, L)) * rng.uniform(0.1, 3.0, size=(N, 1)) + rng.normal(size=(N, 1)) * 5
    cuts = np.sort(rng.choice(np.arange(1, L), size=7, replace=False))
    parts = np.split(np.arange(L), cuts)
    parts.append(np.array([L - 1]))                   # a part of one pixel (cov 0/0) ...
    parts[-2] = parts[-2][:-1]
    parts.append(np.array([], dtype=np.int64))        # ... and an empty one
    perm = rng.permutation(L)
    recs = [_record(x[:, perm[p]]) for p in parts]
    got = tiled.merge_stats(recs, N).numpy()
    ref = _record(x).numpy()
    assert got[0] == L
    rel = np.abs(got[1:] - ref[1:]).max() / np.abs(ref[1:]).max()
    assert rel < 1e-12, rel


def test_merge_stats_keeps_a_slot_axis():
    rng = np.random.default_rng(5)
    N = 4
    a, b = rng.normal(size=(N, 50)), rng.normal(size=(N, 70))
    recs = [torch.stack([_record(a[:, :20]), _record(b[:, :30])]), torch.stack([_record(a[:, 20:]), _record(b[:, 30:])])]
    got = tiled.merge_stats(recs, N)
    assert got.shape == (2, 1 + N + N * N)
    assert torch.allclose(got[0], _record(a), rtol=1e-12, atol=1e-12)
    assert torch.allclose(got[1], _record(b), rtol=1e-12, atol=1e-12)


def test_new_exports_are_declared(lib):
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    for name in ("vst_max_frame_pixels", "vst_cwct_stats_code_rect", "vst_cwct_stats_labels_code_rect"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.vst_version() >= 104
    assert lib.vst_max_frame_pixels() == 1 << 26 == tiled.max_frame_pixels()
    assert "VST_MAX_FRAME_PIXELS" in hdr


@pytest.mark.parametrize("rect", [(-4, 0, 8, 8), (0, -4, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (60, 0, 8, 8), (0, 0, 64, 68),
                                  (4, 4, 64, 8)])
def test_bad_rectangles_are_rejected(lib, rect):
    assert lib.vst_cwct_stats_code_rect(FAKE, 64, 64, 2, *rect, FAKE, FAKE, None) == -1
    assert lib.vst_cwct_stats_code_rect(FAKE, 64, 64, 1, *rect, FAKE, FAKE, None) == -1
    assert lib.vst_cwct_stats_labels_code_rect(FAKE, 64, 64, *rect, FAKE, FAKE, 0, FAKE, FAKE, None) == -1


def test_odd_rectangles_of_artistic_codes_are_rejected(lib):
    assert lib.vst_cwct_stats_code_rect(FAKE, 64, 64, 1, 1, 0, 8, 8, FAKE, FAKE, None) == -1
    assert lib.vst_cwct_stats_code_rect(FAKE, 64, 64, 1, 0, 0, 8, 7, FAKE, FAKE, None) == -1
    assert lib.vst_cwct_stats_code_rect(None, 64, 64, 2, 0, 0, 8, 8, FAKE, FAKE, None) == -1
    assert lib.vst_cwct_stats_code_rect(FAKE, 64, 64, 2, 0, 0, 8, 8, FAKE, None, None) == -4
    assert lib.vst_cwct_stats_code_rect(FAKE, 64, 64, 3, 0, 0, 8, 8, FAKE, FAKE, None) == -3


@pytest.mark.parametrize("H,W", [(16384, 16384), (8196, 8192), (8, (1 << 23) + 4)])
def test_whole_frame_guard_returns_shape_error_before_touching_memory(lib, H, W):
    """Past VST_MAX_FRAME_PIXELS every frame-shaped entry point returns VST_E_SHAPE (-2) on its argument check."""
    net = _lib.NetWeights()
    B = 1
    assert lib.vst_revnet_encode_u8(C.byref(net), FAKE, FAKE, FAKE, B, H, W, 0, None) == -2
    assert lib.vst_revnet_forward_u8(C.byref(net), FAKE, FAKE, FAKE, B, H, W, 2, 0, None) == -2
    assert lib.vst_revnet_inverse(C.byref(net), FAKE, FAKE, FAKE, B, 3, H, W, 2, 0, None) == -2
    assert lib.vst_revnet_decode_u8(C.byref(net), FAKE, FAKE, FAKE, FAKE, B, H, W, 2, 0, None) == -2
    assert lib.vst_cwct_stats_code(FAKE, H, W, 2, FAKE, FAKE, None) == -2
    assert lib.vst_cwct_stats_code_rect(FAKE, H, W, 2, 0, 0, 8, 8, FAKE, FAKE, None) == -2
    assert lib.vst_mask_to_code(FAKE, FAKE, H, W, None) == -2
    assert lib.vst_spread(FAKE, FAKE, FAKE, B, H, W, 2, None) == -2
    assert lib.vst_pass_sub_batch(B, H, W) == -2


def test_largest_whole_frame_passes_the_guard(lib):
    assert lib.vst_pass_sub_batch(1, 8192, 8192) == 1
    assert lib.vst_pass_sub_batch(1, 8, 1 << 23) == 1        # 2^26 pixels in any shape
    assert lib.vst_pass_sub_batch(1, 8, (1 << 23) + 4) == -2


def test_python_guard_names_the_tiled_api(monkeypatch):
    from vstnet_amd import revresnet
    with pytest.raises(RuntimeError, match="stylize_tiled"):
        revresnet._check_frame(16384, 16384)
    revresnet._check_frame(8192, 8192)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        revresnet._check_frame(8190, 8192)
