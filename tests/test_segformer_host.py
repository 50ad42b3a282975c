"""Host-side checks of the segmenter: the state-dict contract, the fp64 decode-head fold, the torch restatement against the
goldens, the scripts' --auto_seg arguments and the ABI."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import segformer_ref as R                                              # noqa: E402

SEED = 4321


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "segformer.npz")))
    g.update(np.load(os.path.join(REPO, "tests", "golden", "segformer_large.npz")))
    g.update(np.load(os.path.join(REPO, "tests", "golden", "segformer_logits.npz")))
    return g


def test_state_dict_spec_is_the_reference_models(golden):
    from vstnet_amd.synth import segformer_state_dict_spec, synthetic_segformer_state_dict
    spec = segformer_state_dict_spec((1, 1, 1, 1), 768)
    assert [k for k, _ in spec] == list(golden["keys"])
    assert [",".join(str(d) for d in s) for _, s in spec] == list(golden["shapes"])
    sd = synthetic_segformer_state_dict(SEED, (1, 1, 1, 1))
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for _, s in spec]
    for k, v in sd.items():
        if v.dtype.is_floating_point and v.ndim == 1:
            assert float(v.abs().min()) > 0, k                       # no zero biases, no unit norm weights
            if k.endswith("weight"):
                assert not torch.all(v == 1) and abs(float(v.mean()) - 1) < 0.05, k
    assert float(sd["decode_head.linear_fuse.bn.running_var"].min()) > 0
    again = synthetic_segformer_state_dict(SEED, (1, 1, 1, 1))
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    b4 = segformer_state_dict_spec()
    assert sum(k.endswith("attn.q.weight") for k, _ in b4) == 3 + 8 + 27 + 3


def test_variants_and_state_dict_errors():
    from vstnet_amd.segformer import check_state_dict
    from vstnet_amd.synth import SEG_DEPTHS, synthetic_segformer_state_dict
    assert SEG_DEPTHS["b4"] == (3, 8, 27, 3) and "b0" not in SEG_DEPTHS and sorted(SEG_DEPTHS) == ["b1", "b2", "b3", "b4", "b5"]
    sd = synthetic_segformer_state_dict(SEED, (1, 1, 1, 1))
    check_state_dict(dict(sd, label_mapping=torch.zeros(3, 150)), (1, 1, 1, 1), 768)
    trimmed = {k: v for k, v in sd.items() if "conv_seg" not in k and "num_batches" not in k}
    check_state_dict(trimmed, (1, 1, 1, 1), 768)
    with pytest.raises(KeyError, match="backbone.block3.0.attn.sr.bias"):
        check_state_dict({k: v for k, v in sd.items() if k != "backbone.block3.0.attn.sr.bias"}, (1, 1, 1, 1), 768)
    with pytest.raises(ValueError, match="backbone.norm2.weight"):
        check_state_dict(dict(sd, **{"backbone.norm2.weight": torch.ones(64)}), (1, 1, 1, 1), 768)
    with pytest.raises(KeyError, match="backbone.block1.1.norm1.weight"):
        check_state_dict(sd, (2, 1, 1, 1), 768)


def test_fp64_head_fold_equals_the_unfolded_head():
    from vstnet_amd.segformer import fold_decode_head
    from vstnet_amd.synth import synthetic_segformer_state_dict
    sd = R.cast(synthetic_segformer_state_dict(SEED, (1, 1, 1, 1)), torch.float64)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn((c, h, w), generator=g, dtype=torch.float64) for c, (h, w) in zip(R.DIMS, ((18, 26), (9, 13), (5, 7), (3, 4)))]
    folded = {k: torch.from_numpy(v) for k, v in fold_decode_head(sd).items()}
    a, b = R.decode_head(sd, xs), R.folded_head(folded, sd, xs)
    assert a.shape == (150, 18, 26)
    assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max())


def test_library_tensor_layouts():
    from vstnet_amd.segformer import library_tensors
    from vstnet_amd.synth import synthetic_segformer_state_dict
    sd = synthetic_segformer_state_dict(SEED, (1, 1, 1, 1))
    t = library_tensors(sd, (1, 1, 1, 1))
    w = sd["backbone.patch_embed1.proj.weight"]
    assert np.array_equal(t["backbone.patch_embed1.proj.weight"].reshape(64, 7, 7, 3)[5, 2, 3, 1], w[5, 1, 2, 3].numpy())
    d = sd["backbone.block2.0.mlp.dwconv.dwconv.weight"]
    assert np.array_equal(t["backbone.block2.0.mlp.dwconv.dwconv.weight"].reshape(9, 512)[5, 17], d[17, 0, 1, 2].numpy())
    assert "decode_head.linear_fuse.conv.weight" not in t and t["decode_head.fold_c3.weight"].size == 768 * 320


@pytest.mark.parametrize("case", ["small", "pad", "chain"])
def test_reference_restatement_reproduces_the_goldens(golden, case):
    from vstnet_amd.synth import synthetic_segformer_state_dict
    depths = tuple(int(d) for d in golden[f"{case}.depths"])
    r = R.segment(synthetic_segformer_state_dict(SEED, depths), golden[f"{case}.frame"], depths, torch.float64)
    assert np.array_equal(r["labels"].numpy(), golden[f"{case}.labels"])
    assert np.abs(r["logits"][:, ::4, ::4].numpy() - golden[f"{case}.logits_s4"]).max() <= 1e-10
    if case == "small":
        for i, x in enumerate(r["xs"]):
            assert np.abs(x.numpy() - golden[f"small.x{i + 1}"]).max() <= 1e-10
        assert golden["small.logits"].dtype == np.float64 and np.abs(r["logits"].numpy() - golden["small.logits"]).max() <= 1e-10
    # the fixtures are not degenerate (the maker asserts the same)
    assert int(golden[f"{case}.labels_2pct"]) >= 4 and float(golden[f"{case}.share_close"]) <= 0.01


def test_fixture_conditions_are_recorded(golden):
    for case in ("small", "pad", "chain", "large"):
        e32, scale = float(golden[f"{case}.e32"]), float(golden[f"{case}.max_logit"])
        close = float((golden[f"{case}.margin"].astype(np.float64) <= 2 * 8 * e32 * scale).mean())
        _, counts = np.unique(golden[f"{case}.labels"], return_counts=True)
        assert close <= 0.01 and int((counts >= 0.02 * golden[f"{case}.labels"].size).sum()) >= 4
        assert 1e-8 < e32 < 1e-5


@pytest.mark.parametrize("script", ["image_transfer", "video_transfer"])
def test_scripts_parse_auto_seg(script, capsys, tmp_path):
    mod = __import__(script)
    p = mod.build_parser()
    base = ["--content", "c.png", "--style", "s.png"] if script == "image_transfer" else ["--video", "v", "--style", "s.png"]
    table = tmp_path / "rel.npy"
    np.save(table, np.zeros((3, 150), np.int16))
    ok = base + ["--auto_seg", "--synthetic_seg_weights", "--label_mapping", str(table)]
    a = p.parse_args(ok)
    assert a.auto_seg and a.synthetic_seg_weights and a.seg_variant == "b4" and a.seg_ckpoint is None and not a.no_seg_remap
    mod.check_seg_args(p, a)
    mod.check_seg_args(p, p.parse_args(base + ["--auto_seg", "--seg_ckpoint", "w.pth", "--seg_variant", "b2", "--no_seg_remap"]))

    def rejected(argv, word):
        with pytest.raises(SystemExit) as e:
            mod.check_seg_args(p, p.parse_args(argv))
        assert e.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(ok + ["--seg_variant", "b0"])
    capsys.readouterr()
    rejected(base + ["--auto_seg", "--no_seg_remap"], "--seg_ckpoint")
    rejected(base + ["--auto_seg", "--synthetic_seg_weights", "--label_mapping", str(tmp_path / "none.npy")], "--no_seg_remap")
    rejected(ok + ["--interpolate_labels"], "--interpolate_labels")
    rejected(ok + ["--content_seg", "c.png"], "--content_seg")
    rejected(ok + ["--styles", "a.png", "b.png"], "--styles")
    if script == "video_transfer":
        rejected(ok + ["--content_seg_dir", "d"], "--content_seg_dir")
        rejected(ok + ["--alpha_s_end", "1.0"], "--alpha_s_end")
        rejected(ok + ["--mode", "artistic"], "photorealistic")
    else:
        mod.check_seg_args(p, p.parse_args(ok + ["--mode", "artistic"]))


def test_abi_exports():
    from vstnet_amd import _lib
    names = ["vst_seg_create", "vst_seg_tensor_count", "vst_seg_tensor_info", "vst_seg_load_tensor", "vst_seg_run_u8",
             "vst_seg_logits", "vst_seg_shape", "vst_seg_destroy"]
    assert all(n in _lib.EXPORTS for n in names)
    header = open(os.path.join(REPO, "include", "vstnet.h")).read()
    assert all(f"int {n}(" in header for n in names)
    if os.path.exists(_lib.LIB_PATH):
        import ctypes as C
        L = _lib.lib()
        assert all(hasattr(L, n) for n in names)
        hw = (C.c_int * 8)()
        assert L.vst_seg_shape(72, 104, hw) == 0 and list(hw) == [18, 26, 9, 13, 5, 7, 3, 4]
        assert L.vst_seg_shape(31, 104, hw) == -2 and L.vst_seg_shape(104, 31, hw) == -2
        assert L.vst_seg_shape(720, 1280, hw) == 0 and list(hw)[:2] == [180, 320]
