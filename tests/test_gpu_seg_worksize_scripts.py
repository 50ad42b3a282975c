"""`image_transfer.py` and `video_transfer.py` with `--auto_seg --seg_size` end to end on the GPU (MiT-B1, synthetic weights, maps
used as segmented): the label maps written are those of segment_u8(..., work_size=...), and the stylised frames are those of the
library fed these maps."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from vstnet_amd.synth import SEG_DEPTHS, synthetic_scene_u8, synthetic_segformer_state_dict

pytestmark = pytest.mark.gpu
S = 104
SEG_FLAGS = ["--auto_seg", "--synthetic_seg_weights", "--seg_variant", "b1", "--seg_size", str(S), "--no_seg_remap"]


@pytest.fixture(scope="module")
def segmenter():
    from vstnet_amd.segformer import SegFormer
    return SegFormer("b1", embedding_dim=256).load_state_dict(synthetic_segformer_state_dict(4321, SEG_DEPTHS["b1"], 256))


def work_map(segmenter, img_u8):
    return segmenter.segment_u8(torch.from_numpy(np.ascontiguousarray(img_u8)).cuda(), work_size=S).cpu().numpy()


def test_image_transfer_seg_size(tmp_path, segmenter):
    import image_transfer
    from models.cWCT import cWCT
    c, s = synthetic_scene_u8(144, 208, 31), synthetic_scene_u8(128, 176, 32)
    Image.fromarray(c).save(tmp_path / "c.png")
    Image.fromarray(s).save(tmp_path / "s.png")
    out = image_transfer.main(["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--synthetic_weights",
                               "--out_dir", str(tmp_path / "o")] + SEG_FLAGS)
    cm, sm = work_map(segmenter, c), work_map(segmenter, s)
    seg_dir = tmp_path / "o" / "segmentation"
    assert np.array_equal(np.asarray(Image.open(seg_dir / "content_seg_label.png")), cm)
    assert np.array_equal(np.asarray(Image.open(seg_dir / "style_seg_label.png")), sm)
    assert len(np.unique(cm)) >= 2
    plain = segmenter.segment_u8(torch.from_numpy(c).cuda()).cpu().numpy()
    assert not np.array_equal(cm, plain)                    # (the flag did something)
    net = image_transfer.build_network("photorealistic", None, True, torch.device("cuda"))
    want = image_transfer.stylize(net, cWCT(), Image.fromarray(c), Image.fromarray(s), cm[None], sm[None])
    got = np.asarray(Image.open(out))
    assert got.shape == (144, 208, 3) and np.array_equal(got, want) and not np.array_equal(got, c)
    # the host route of the tiled branch: PIL's resize and an upload of the working copy give the same maps
    host = image_transfer.segment_image(segmenter, Image.fromarray(c), S, torch.device("cuda"), host_resize=True)
    assert np.array_equal(host.cpu().numpy(), cm)


def test_video_transfer_seg_size(tmp_path, segmenter):
    """Three frames: the frames written equal those of the same script fed, from files, the maps segment_u8(work_size=S) returns
    (the per-frame mask route), and the maps written are these maps."""
    import video_transfer
    fd, md = tmp_path / "clip", tmp_path / "maps"
    fd.mkdir()
    md.mkdir()
    frames = [synthetic_scene_u8(144, 208, 40 + i) for i in range(3)]
    style = synthetic_scene_u8(128, 176, 50)
    maps, sm = [work_map(segmenter, f) for f in frames], work_map(segmenter, style)
    for i, (f, m) in enumerate(zip(frames, maps)):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
        Image.fromarray(m, mode="L").save(md / f"{i:03d}.png")
    Image.fromarray(style).save(tmp_path / "s.png")
    Image.fromarray(sm, mode="L").save(tmp_path / "sseg.png")
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only"]
    auto = video_transfer.main(base + SEG_FLAGS + ["--out_dir", str(tmp_path / "o1")])
    files = video_transfer.main(base + ["--content_seg_dir", str(md), "--style_seg", str(tmp_path / "sseg.png"),
                                        "--out_dir", str(tmp_path / "o0")])
    names = ["%05d.png" % i for i in range(3)]
    assert sorted(os.listdir(auto)) == sorted(os.listdir(files)) == names
    seg_dir = tmp_path / "o1" / "segmentation"
    assert np.array_equal(np.asarray(Image.open(seg_dir / "style_seg_label.png")), sm)
    for i, n in enumerate(names):
        got = np.asarray(Image.open(os.path.join(auto, n)))
        assert np.array_equal(got, np.asarray(Image.open(os.path.join(files, n)))), n
        assert not np.array_equal(got, frames[i])
        assert np.array_equal(np.asarray(Image.open(seg_dir / ("%05d_label.png" % i))), maps[i]), i
    plain = segmenter.segment_u8(torch.from_numpy(frames[0]).cuda()).cpu().numpy()
    assert not np.array_equal(maps[0], plain)               # (the flag did something)
