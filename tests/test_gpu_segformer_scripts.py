"""`image_transfer.py --auto_seg` and `video_transfer.py --auto_seg` end to end on the GPU (MiT-B1, synthetic weights, a real
relation table): the label maps written are the host SegReMapping of what the segmenter returns, and the stylised frames are
those of the same scripts fed these maps from files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from vstnet_amd.synth import SEG_DEPTHS, synthetic_scene_u8, synthetic_segformer_state_dict

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_FLAGS = ["--auto_seg", "--synthetic_seg_weights", "--seg_variant", "b1"]


@pytest.fixture(scope="module")
def table():
    return np.load(os.path.join(REPO, "tests", "golden", "segremap.npz"))["mapping"]


@pytest.fixture(scope="module")
def segmenter():
    from vstnet_amd.segformer import SegFormer
    return SegFormer("b1", embedding_dim=256).load_state_dict(synthetic_segformer_state_dict(4321, SEG_DEPTHS["b1"], 256))


def raw_map(segmenter, img_u8):
    return segmenter.segment_u8(torch.from_numpy(np.ascontiguousarray(img_u8)).cuda()).cpu().numpy()


def test_image_transfer_auto_seg(tmp_path, table, segmenter):
    import image_transfer
    from models.segmentation.SegReMapping import SegReMapping
    c, s = synthetic_scene_u8(72, 104, 31), synthetic_scene_u8(64, 88, 32)
    Image.fromarray(c).save(tmp_path / "c.png")
    Image.fromarray(s).save(tmp_path / "s.png")
    np.save(tmp_path / "rel.npy", table)
    np.save(tmp_path / "pal.npy", (np.arange(150 * 3).reshape(150, 3) % 256).astype(np.uint8))
    base = ["--content", str(tmp_path / "c.png"), "--style", str(tmp_path / "s.png"), "--synthetic_weights"]
    out = image_transfer.main(base + SEG_FLAGS + ["--label_mapping", str(tmp_path / "rel.npy"), "--palette", str(tmp_path / "pal.npy"),
                                                  "--out_dir", str(tmp_path / "o")])
    host = SegReMapping(table.astype(np.int64), 0.01)
    sm = host.self_remapping(raw_map(segmenter, s))
    cm = host.cross_remapping(host.self_remapping(raw_map(segmenter, c)), sm)
    seg_dir = tmp_path / "o" / "segmentation"
    assert np.array_equal(np.asarray(Image.open(seg_dir / "content_seg_label.png")), cm)
    assert np.array_equal(np.asarray(Image.open(seg_dir / "style_seg_label.png")), sm)
    assert np.asarray(Image.open(seg_dir / "content_seg_color.png")).shape == (72, 104, 3)
    assert len(np.unique(cm)) >= 2
    # the script's own stylize() fed the two remapped maps from the host (load_segment would read files as colour maps)
    from models.cWCT import cWCT
    net = image_transfer.build_network("photorealistic", None, True, torch.device("cuda"))
    want = image_transfer.stylize(net, cWCT(), Image.fromarray(c), Image.fromarray(s), cm[None], sm[None])
    got = np.asarray(Image.open(out))
    assert got.shape == (72, 104, 3) and np.array_equal(got, want) and not np.array_equal(got, c)


def test_video_transfer_auto_seg_and_two_shards(tmp_path, table, segmenter):
    import video_transfer
    from models.segmentation.SegReMapping import SegReMapping
    fd, sd_ = tmp_path / "clip", tmp_path / "segs"
    fd.mkdir()
    sd_.mkdir()
    frames = [synthetic_scene_u8(64, 96, 40 + i) for i in range(4)]
    style = synthetic_scene_u8(72, 104, 50)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(fd / f"{i:03d}.png")
        Image.fromarray(raw_map(segmenter, f), mode="L").save(sd_ / f"{i:03d}.png")
    Image.fromarray(style).save(tmp_path / "s.png")
    Image.fromarray(raw_map(segmenter, style), mode="L").save(tmp_path / "sseg.png")
    np.save(tmp_path / "rel.npy", table)
    base = ["--video", str(fd), "--style", str(tmp_path / "s.png"), "--synthetic_weights", "--frames_only",
            "--label_mapping", str(tmp_path / "rel.npy")]
    auto = video_transfer.main(base + SEG_FLAGS + ["--out_dir", str(tmp_path / "o1")])
    files = video_transfer.main(base + ["--content_seg_dir", str(sd_), "--style_seg", str(tmp_path / "sseg.png"), "--seg_remap",
                                        "--out_dir", str(tmp_path / "o0")])
    names = ["%05d.png" % i for i in range(4)]
    assert sorted(os.listdir(auto)) == sorted(os.listdir(files)) == names
    for n in names:
        assert np.array_equal(np.asarray(Image.open(os.path.join(auto, n))), np.asarray(Image.open(os.path.join(files, n)))), n
    host = SegReMapping(table.astype(np.int64), 0.01)
    sm = host.self_remapping(raw_map(segmenter, style))
    seg_dir = tmp_path / "o1" / "segmentation"
    assert np.array_equal(np.asarray(Image.open(seg_dir / "style_seg_label.png")), sm)
    for i, f in enumerate(frames):
        want = host.cross_remapping(host.self_remapping(raw_map(segmenter, f)), sm)
        assert np.array_equal(np.asarray(Image.open(seg_dir / ("%05d_label.png" % i))), want), i
    # two shards: the parent never touches the GPU, every child segments and writes its own frames
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "video_transfer.py")] + base + SEG_FLAGS
                       + ["--out_dir", str(tmp_path / "o2"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    multi = os.path.join(str(tmp_path / "o2"), os.path.basename(auto))
    for n in names:
        assert np.array_equal(np.asarray(Image.open(os.path.join(auto, n))), np.asarray(Image.open(os.path.join(multi, n)))), n
    for i in range(4):
        a, b = seg_dir / ("%05d_label.png" % i), tmp_path / "o2" / "segmentation" / ("%05d_label.png" % i)
        assert np.array_equal(np.asarray(Image.open(a)), np.asarray(Image.open(b))), i
