"""CPU: per-frame segmentation masks - the exports of csrc/masks.hip, the argument handling of
`video_transfer.py --content_seg_dir`, and the numpy model of the remap-table and plan kernels (vstnet_amd/masks.py: their
specification) against models.segmentation.SegReMapping and the validity rule."""
import os
import re

import numpy as np
import pytest
from PIL import Image

from vstnet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["vst_colors_to_labels", "vst_label_hist", "vst_mask_prepare", "vst_remap_lut", "vst_apply_lut",
               "vst_label_plan_hist", "vst_cwct_factor_labels_keyed"]
E_ARG, E_SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_and_exports_agree_with_the_new_symbols(lib):
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    declared = set(re.findall(r"\b(vst_[a-z0-9_]+)\s*\(", hdr)) - {"vst_conv_weights", "vst_block_weights", "vst_net_weights"}
    assert declared == set(_lib.EXPORTS)
    for name in NEW_EXPORTS:
        assert name in declared and hasattr(lib, name), name
    assert "VST_MASK_OVERFLOW 1u" in hdr and "VST_MASK_OUT_OF_TABLE 2u" in hdr
    assert (_lib.MASK_OVERFLOW, _lib.MASK_OUT_OF_TABLE) == (1, 2)


def test_arguments_are_validated_before_any_launch(lib):
    import ctypes as C
    p = C.c_void_p(64)          # never dereferenced: every call below must fail on its arguments
    z = C.c_void_p(0)
    assert lib.vst_colors_to_labels(z, p, 16, z) == E_ARG and lib.vst_colors_to_labels(p, p, 0, z) == E_ARG
    assert lib.vst_label_hist(p, 16, z, z) == E_ARG
    assert lib.vst_mask_prepare(z, 0, 8, 8, p, p, z) == E_ARG
    assert lib.vst_mask_prepare(p, 0, 8, 10, p, p, z) == E_SHAPE and lib.vst_mask_prepare(p, 1, 4, 8, p, p, z) == E_SHAPE
    assert lib.vst_mask_prepare(C.c_void_p(66), 0, 8, 8, p, p, z) == E_ARG          # dword loads need alignment
    assert lib.vst_remap_lut(p, z, z, 150, 150, 1, p, z, z, z) == E_ARG
    assert lib.vst_remap_lut(p, z, p, 0, 150, 1, p, z, z, z) == E_SHAPE
    assert lib.vst_remap_lut(p, z, p, 150, 150, -1, p, z, z, z) == E_ARG
    assert lib.vst_apply_lut(p, z, p, 16, z) == E_ARG
    assert lib.vst_label_plan_hist(p, z, p, 0, p, z, z) == E_SHAPE and lib.vst_label_plan_hist(p, z, p, 33, p, z, z) == E_SHAPE
    assert lib.vst_label_plan_hist(z, z, p, 8, p, z, z) == E_ARG
    assert lib.vst_cwct_factor_labels_keyed(p, p, p, z, 8, 2e-5, 32, p, p, z) == E_ARG
    assert lib.vst_cwct_factor_labels_keyed(p, p, p, p, 8, 2e-5, 16, p, p, z) == E_SHAPE


# ------------------------------------------------------------------------------------------------ the model of the kernels
def _host_chain(remap, seg, sty_self):
    return remap.cross_remapping(remap.self_remapping(seg), sty_self)


def _model_chain(table, min_ratio, seg, sty_self):
    from vstnet_amd import masks
    hist = np.bincount(seg.reshape(-1), minlength=256)
    lut, h2, flags = masks.remap_lut_model(hist, table, masks.min_count(seg.size, min_ratio),
                                           np.bincount(sty_self.reshape(-1), minlength=256))
    out = lut[seg]
    assert flags == 0 and np.array_equal(h2, np.bincount(out.reshape(-1), minlength=256))
    return out, lut, hist


def test_model_matches_segremapping_on_the_golden_cases():
    from models.segmentation.SegReMapping import SegReMapping
    from vstnet_amd import masks
    g = np.load(os.path.join(REPO, "tests", "golden", "segremap.npz"))
    table, ratio = g["mapping"], float(g["min_ratio"])
    host = SegReMapping(table.astype(np.int64), ratio)
    for t in range(int(g["n_cases"])):
        seg, sty = g[f"seg_{t}"], g[f"sty_{t}"]
        for m in (seg, sty):          # self_remapping alone
            lut, _, fl = masks.remap_lut_model(np.bincount(m.reshape(-1), minlength=256), table, masks.min_count(m.size, ratio))
            assert fl == 0 and np.array_equal(lut[m], host.self_remapping(m))
        assert np.array_equal(lut[sty], g[f"self_sty_{t}"])
        out, lut, hist = _model_chain(table, ratio, seg, g[f"self_sty_{t}"])
        assert np.array_equal(out, g[f"cross_{t}"]) and np.array_equal(out, _host_chain(host, seg, g[f"self_sty_{t}"]))
        # the plan from histograms == the validity rule on the remapped maps, slots in increasing label order
        hs = np.bincount(g[f"self_sty_{t}"].reshape(-1), minlength=256)
        n, over, plan_lut, slot_label = masks.plan_model(hist, lut, hs, 8)
        hc = np.bincount(out.reshape(-1), minlength=256)
        want = [l for l in range(256) if hc[l] > 10 and hs[l] > 10 and hc[l] / hs[l] < 100 and hs[l] / hc[l] < 100]
        assert slot_label == want[:8] and n == len(want[:8]) and over == (len(want) > 8)
        slot_of = {l: k for k, l in enumerate(slot_label)}
        assert np.array_equal(plan_lut[seg], np.vectorize(lambda l: slot_of.get(int(l), 255))(out).astype(np.uint8))


@pytest.mark.parametrize("shape,min_ratio", [((48, 64), 0.01), ((100, 100), 0.01), ((1080, 1920), 0.01), ((37, 53), 0.03),
                                              ((64, 64), 1.0 / 3.0)])
def test_model_decides_like_the_host_class_at_the_threshold(shape, min_ratio):
    """maps built to sit exactly at count == threshold and threshold - 1"""
    from models.segmentation.SegReMapping import SegReMapping
    from vstnet_amd import masks
    g = np.load(os.path.join(REPO, "tests", "golden", "segremap.npz"))
    table = g["mapping"]
    host = SegReMapping(table.astype(np.int64), min_ratio)
    n = shape[0] * shape[1]
    thr = masks.min_count(n, min_ratio)
    assert 1 <= thr <= n
    assert not (np.float32(thr) / n < min_ratio) and (np.float32(thr - 1) / n < min_ratio)
    small = 7
    big = int(table[0, small]) if int(table[0, small]) != small else int(table[1, small])
    for count, moves in ((thr, False), (thr - 1, True)):
        if count == 0:
            continue
        seg = np.full(n, big, np.uint8)
        seg[:count] = small
        seg = seg.reshape(shape)
        want = host.self_remapping(seg)
        lut, _, _ = masks.remap_lut_model(np.bincount(seg.reshape(-1), minlength=256), table, thr)
        assert np.array_equal(lut[seg], want)
        assert (int(want.reshape(-1)[0]) != small) == moves
    # the candidate's own share at the boundary: `small` is under the ratio, its first related label has threshold - 1 or threshold
    for count in (thr - 1, thr):
        if count < 1 or 1 + count >= n:
            continue
        seg = np.full(n, 120, np.uint8)
        seg[0] = small
        seg[1:1 + count] = big
        seg = seg.reshape(shape)
        lut, _, _ = masks.remap_lut_model(np.bincount(seg.reshape(-1), minlength=256), table, thr)
        assert np.array_equal(lut[seg], host.self_remapping(seg))


def test_model_flags_a_label_outside_the_table():
    from models.segmentation.SegReMapping import SegReMapping
    from vstnet_amd import masks
    table = np.load(os.path.join(REPO, "tests", "golden", "segremap.npz"))["mapping"]
    seg = np.zeros((40, 40), np.uint8)
    seg[0, :3] = 200                                   # under the ratio and >= cols
    with pytest.raises(IndexError):
        SegReMapping(table.astype(np.int64), 0.01).self_remapping(seg)
    lut, _, flags = masks.remap_lut_model(np.bincount(seg.reshape(-1), minlength=256), table, masks.min_count(seg.size, 0.01))
    assert flags == masks.OUT_OF_TABLE and lut[200] == 200


def test_plan_model_caps_the_slots():
    from vstnet_amd import masks
    hist = np.zeros(256, np.int64)
    hist[10:20] = 100
    n, over, lut, labels = masks.plan_model(hist, None, hist, 8)
    assert (n, over, labels) == (8, True, list(range(10, 18))) and lut[18] == 255 and lut[10] == 0
    n, over, lut, labels = masks.plan_model(hist, None, hist, 32)
    assert (n, over, labels) == (10, False, list(range(10, 20)))


# ------------------------------------------------------------------------------------------------ the script's host logic
COLOURS = {0: (0, 0, 0), 1: (255, 255, 255), 2: (0, 255, 0), 3: (0, 0, 255), 4: (255, 0, 0)}


def _clip(tmp_path, n=6, size=(32, 24)):
    vid, segs = tmp_path / "clip", tmp_path / "segs"
    vid.mkdir()
    segs.mkdir()
    rng = np.random.RandomState(0)
    for i in range(n):
        Image.fromarray(rng.randint(0, 255, (size[1], size[0], 3), dtype=np.uint8)).save(vid / f"{i:03d}.png")
        m = np.zeros((size[1], size[0], 3), np.uint8)
        m[:, : 4 + 3 * i] = COLOURS[1 + i % 3]           # three different maps, shifted per frame
        if i % 2:
            Image.fromarray(m).save(segs / f"{i:03d}.png")
        else:                                            # a single-channel label PNG
            lab = np.zeros((size[1], size[0]), np.uint8)
            lab[:, : 4 + 3 * i] = 1 + i % 3
            Image.fromarray(lab, mode="L").save(segs / f"{i:03d}.png")
    Image.fromarray(rng.randint(0, 255, (24, 32, 3), dtype=np.uint8)).save(tmp_path / "style.png")
    sseg = np.zeros((24, 32, 3), np.uint8)
    sseg[:, :16] = COLOURS[1]
    Image.fromarray(sseg).save(tmp_path / "style_seg.png")
    return vid, segs


def _argv(tmp_path, vid, segs, *more):
    return ["--video", str(vid), "--style", str(tmp_path / "style.png"), "--style_seg", str(tmp_path / "style_seg.png"),
            "--content_seg_dir", str(segs), "--out_dir", str(tmp_path / "out"), "--stub_stylise", "--frames_only",
            "--workers", "1", *more]


def test_content_seg_dir_arguments(tmp_path):
    import video_transfer as vt
    vid, segs = _clip(tmp_path)
    with pytest.raises(SystemExit, match="mutually exclusive"):
        vt.main(_argv(tmp_path, vid, segs, "--content_seg", str(tmp_path / "style_seg.png")))
    with pytest.raises(SystemExit, match="photorealistic"):
        vt.main(_argv(tmp_path, vid, segs, "--mode", "artistic"))
    os.remove(segs / "005.png")
    with pytest.raises(SystemExit, match="5 maps for 6 frames"):
        vt.main(_argv(tmp_path, vid, segs))
    with pytest.raises(SystemExit, match="--seg_remap"):
        vt.main(["--video", str(vid), "--style", str(tmp_path / "style.png"), "--out_dir", str(tmp_path / "out"), "--stub_stylise",
                 "--seg_remap"])


def test_shards_take_their_own_maps(tmp_path):
    import video_transfer as vt
    vid, segs = _clip(tmp_path)
    table = tmp_path / "rel.npy"
    np.save(table, np.load(os.path.join(REPO, "tests", "golden", "segremap.npz"))["mapping"])
    seen = {}
    for r in range(3):
        out = vt.main(_argv(tmp_path, vid, segs, "--shard", f"{r}/3", "--seg_remap", "--label_mapping", str(table)))
        assert sorted(vt.LAST_RUN["masks"]) == [2 * r, 2 * r + 1] and vt.LAST_RUN["redo"] == 0
        seen.update(vt.LAST_RUN["masks"])
    assert [os.path.basename(seen[i]) for i in range(6)] == [f"{i:03d}.png" for i in range(6)]
    assert sorted(os.listdir(out)) == [f"{i:05d}.png" for i in range(6)]
    # both kinds of file arrive as what the device takes: labels for L / P files, colours for RGB files, at the frame's size
    lab, col = vt.load_frame_mask(seen[0], (16, 12)), vt.load_frame_mask(seen[1], (16, 12))
    assert lab.shape == (12, 16) and lab.dtype == np.uint8 and set(np.unique(lab)) <= {0, 1}
    assert col.shape == (12, 16, 3) and tuple(col[0, 0]) == COLOURS[2]
