"""The style loss as a chain (vstnet_amd.vgg.StyleLoss, models.VGG.VGG19) against what the reference's own code returns
(tests/golden/vgg.npz, written by tests/make_vgg_golden.py).

Bound, for loss_s, loss_c and each of the eight record groups (per tap the means and the stds, max error over max value):

    |device - f64| / |f64|  <=  FACTOR x max(e32, FLOOR)

e32 = the golden's fp32 value against its fp64 value under the same metric; FLOOR = 8 u because a scalar from one fp32 run can
land within 1 u of the truth by luck (tests/test_vgg_host.py shows one that did); FACTOR = 8 has its teeth shown there: the
fp32 host restatement of the device arithmetic stays under FACTOR / 2 and every mutant of tests/vgg_ref.py is over 1.25 FACTOR.

Measured on the MI355X (device / max(e32, floor), worst figure per case; the u8 and the f32 entry give the same bits):
9x9 0.66 (relu4_1 std; loss_s 0.15, loss_c 0.19), 17x23 0.63 (relu4_1 std; loss_s 0.08, loss_c 0.46), 32x48 0.87 (relu4_1 std;
loss_s 0.12, loss_c 0.35).  test_golden_cases prints all ten figures per case."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import vgg_ref as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden):
    return golden("vgg")


@pytest.fixture(scope="module")
def sd(gold):
    return R.weights(int(gold["weight_seed"]))


@pytest.fixture(scope="module")
def encoder(sd):
    from vstnet_amd.vgg import VGGEncoder
    return VGGEncoder(sd, "cuda:0")


def as_entry(img_u8, entry):
    """the device tensor of an image for the u8 entry ([h,w,3] bytes) or the f32 entry ([3,h,w] of v / 255)"""
    t = torch.from_numpy(np.ascontiguousarray(img_u8))
    return t.cuda() if entry == "u8" else (t.permute(2, 0, 1).float() / 255.0).contiguous().cuda()


@pytest.mark.parametrize("entry", ["u8", "f32"])
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_golden_cases(encoder, gold, case, entry):
    """the reference's loss_s, loss_c and records; the style has another size than the frame in every case, and 9x9 is the
    smallest legal frame"""
    from vstnet_amd.vgg import StyleLoss
    frame, style, content = R.case_images(case)
    assert frame.shape[:2] != style.shape[:2]
    meter = StyleLoss(encoder, as_entry(style, entry))
    both = meter(as_entry(frame, entry), as_entry(content, entry)).cpu().numpy().copy()
    rec = meter.records.cpu().numpy().copy()
    alone = meter(as_entry(frame, entry)).cpu().numpy().copy()
    assert both.dtype == np.float64 and both.shape == (2,) and alone.shape == (1,) and alone[0] == both[0]
    r = R.ratios({"loss_s": both[0], "loss_c": both[1], "rec": rec}, gold, case)
    print(f"{case} {entry}: loss_s {both[0]:.9e} loss_c {both[1]:.9e}; device / max(e32, floor): "
          + ", ".join(f"{k} {v:.2f}" for k, v in r.items()))
    assert max(r.values()) <= R.FACTOR, (case, entry, r)


def test_entries_agree_bit_for_bit(encoder):
    """x / 255 is one correctly rounded fp32 division on either side of the edge"""
    from vstnet_amd.vgg import StyleLoss
    frame, style, content = R.case_images("17x23")
    a = StyleLoss(encoder, as_entry(style, "u8"))(as_entry(frame, "u8"), as_entry(content, "u8")).cpu()
    b = StyleLoss(encoder, as_entry(style, "f32"))(as_entry(frame, "f32"), as_entry(content, "f32")).cpu()
    assert torch.equal(a, b)


def test_repeatable_and_out(encoder):
    """fixed reduction orders: the same frame gives the same bits; `out` receives the values; clone() shares the style"""
    from vstnet_amd.vgg import StyleLoss, style_loss
    frame, style, content = R.case_images("32x48")
    meter = StyleLoss(encoder, as_entry(style, "u8"))
    first = meter(as_entry(frame, "u8"), as_entry(content, "u8")).cpu().clone()
    out = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    again = meter.clone()(as_entry(frame, "u8"), as_entry(content, "u8"), out=out)
    assert again.data_ptr() == out.data_ptr() and torch.equal(again.cpu(), first) and float(out[2]) == -1.0
    assert torch.equal(style_loss(encoder, as_entry(frame, "u8"), as_entry(style, "u8"), as_entry(content, "u8")).cpu(), first)
    # a frame against itself as the style
    assert float(StyleLoss(encoder, as_entry(frame, "u8"))(as_entry(frame, "u8"), as_entry(frame, "u8")).cpu().abs().max()) == 0.0


def test_refusals(encoder):
    from vstnet_amd._lib import VstError
    from vstnet_amd.vgg import StyleLoss
    frame, style, content = R.case_images("9x9")
    meter = StyleLoss(encoder, as_entry(style, "u8"))
    small = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(VstError):
        meter(small)
    with pytest.raises(VstError):
        StyleLoss(encoder, small)
    with pytest.raises(VstError):
        meter(torch.zeros((9, 8, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        meter(as_entry(frame, "u8"), as_entry(style, "u8"))          # the content at another size
    with pytest.raises(ValueError):
        meter(torch.from_numpy(frame))                               # a host tensor: no CPU fallback
    assert meter(as_entry(frame, "u8")).shape == (1,)               # and the object still works


def test_models_vgg_equals_style_loss(encoder, sd, gold):
    """the reference's import path: forward is StyleLoss; the per-layer route runs the same kernels one call at a time, so its
    maps are the chain's bits and its losses differ only by the order of a few fp64 additions"""
    from models.VGG import VGG19, calc_mean_std
    from vstnet_amd.vgg import StyleLoss, split_records
    net = VGG19(sd, "cuda:0")
    frame, style, content = R.case_images("17x23")
    f, s, c = (as_entry(i, "f32")[None] for i in (frame, style, content))
    want = StyleLoss(encoder, s[0])(f[0], c[0]).cpu().clone()
    loss_c, loss_s = net(c, s, f, content_weight=1)
    assert float(loss_s) == float(want[0]) and float(loss_c) == float(want[1])
    loss_c0, loss_s0 = net(c, s, f)
    assert loss_c0 == 0 and float(loss_s0) == float(want[0])
    # the per-layer route
    rec, map4 = encoder.features(f[0], relu4_1=True)
    feats = net.encode_with_intermediate(f)
    assert [tuple(t.shape) for t in feats] == [(1, 64, 17, 23), (1, 128, 9, 12), (1, 256, 5, 6), (1, 512, 3, 3)]
    assert torch.equal(net.encode(f), feats[3]) and torch.equal(R.tokens(feats[3].cpu()), map4.cpu())
    for feat, (mean, std) in zip(feats, split_records(rec)):
        m, sdv = calc_mean_std(feat)
        assert tuple(m.shape) == (1, feat.shape[1], 1, 1) and torch.equal(m.reshape(-1), mean) and torch.equal(sdv.reshape(-1), std)
    assert len(net.encode_with_intermediate(f, 2)) == 2
    sf = net.encode_with_intermediate(s)
    by_layer = sum(net.calc_style_loss(a, b) for a, b in zip(feats, sf))
    assert abs(float(by_layer) - float(want[0])) <= 1e-12 * float(want[0])
    assert abs(float(net.calc_content_loss(feats[3], net.encode(c))) - float(want[1])) <= 1e-12 * float(want[1])
    # three layers take the per-layer route inside forward
    _, loss_s3 = net(c, s, f, n_layer=3)
    assert abs(float(loss_s3) - float(sum(net.calc_style_loss(a, b) for a, b in zip(feats[:3], sf[:3])))) <= 1e-15
    with pytest.raises(ValueError, match="relu4_1"):                # (the reference indexes past its list here)
        net(c, s, f, n_layer=3, content_weight=1)
    # a batch: the means over the images, with one style for all or one each; the per-layer weights were made on first use
    two = torch.cat([f, c])
    lc2, ls2 = net(torch.cat([c, f]), s, two, content_weight=1)
    single = [StyleLoss(encoder, s[0])(x[0], y[0]).cpu().clone() for x, y in ((f, c), (c, f))]
    assert float(ls2) == float((single[0][0] / 2 + single[1][0] / 2)) and float(lc2) == float((single[0][1] / 2 + single[1][1] / 2))
    assert float(net(c, torch.cat([s, s]), two)[1]) == float(ls2)
    with pytest.raises(ValueError, match="style images"):
        net(c, torch.cat([s, s, s]), two)
    assert VGG19(sd, "cuda:0")._packed is None and net._packed is not None
    # against the golden too: the drop-in returns the reference's numbers
    assert R.ratios({"loss_s": float(loss_s), "loss_c": float(loss_c)}, gold, "17x23")["loss_s"] <= R.FACTOR
