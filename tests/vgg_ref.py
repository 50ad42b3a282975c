"""Reference, host restatement, mutants and cases of the style-loss tests (test infrastructure only; tests/test_vgg_host.py,
tests/test_gpu_vgg_ops.py, tests/test_gpu_vgg.py, tests/make_vgg_golden.py).

Reference: a torch statement of the reference's VGG-19 encoder up to relu4_1 and of its loss_s / loss_c, at the dtype it is
given (fp64 = the truth; tests/golden/vgg.npz holds what the reference's own code returns, and the fp64 run here agrees with
it to 1e-12).  Mutants: switches that make the statement wrong in one way each; a bound the restatement meets with room and
every mutant misses is a bound with teeth.  Restatement: the device arithmetic in fp32 on the host - the input conv in its
fixed order, every 3 x 3 conv as the six-product split GEMM of tests/segformer_ops_ref.py over the reflect-gathered column
matrix, the reductions in fp64.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
import segformer_ops_ref as O                                          # noqa: E402
from vstnet_amd.synth import VGG_CONVS, VGG_ENCODER_LAST, synthetic_vgg_state_dict    # noqa: E402

U = 2.0 ** -24
FACTOR = 8.0                   # the figure tests/test_gpu_segformer.py uses for whole networks; test_vgg_host.py shows its teeth
FLOOR = 8 * U                  # a scalar from one fp32 run can land within 1 u of the truth by luck
WEIGHT_SEED = 1919
EPS = 1e-5
TAPS = {2: 0, 9: 1, 16: 2, 29: 3}
POOL_AFTER = (5, 12, 25)
LEVEL_CHANNELS = (64, 128, 256, 512)
RECORD_OFFSETS = (0, 128, 384, 896)
MUTANTS = ("zero padding", "floor pooling", "biased variance", "eps = 0", "no 1x1 conv", "std without sqrt")

# (frame size, style size); the content has the frame's size
CASES = {"9x9": ((9, 9), (12, 10)), "17x23": ((17, 23), (16, 24)), "32x48": ((32, 48), (25, 31))}


def image_u8(h, w, seed):
    """seeded uint8 [h][w][3]: smooth colour ramps under noise, so that the taps' statistics differ between images"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = rng.uniform(40, 215, 3)[None, None, :] + rng.uniform(-60, 60, 3)[None, None, :] * (yy / h)[..., None] \
        + rng.uniform(-60, 60, 3)[None, None, :] * (xx / w)[..., None]
    img = base + rng.normal(0, rng.uniform(8, 40), (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def case_images(name):
    """-> (frame, style, content) uint8"""
    (h, w), (hs, ws) = CASES[name]
    k = sorted(CASES).index(name)
    return image_u8(h, w, 100 + 10 * k), image_u8(hs, ws, 101 + 10 * k), image_u8(h, w, 102 + 10 * k)


def weights(seed=WEIGHT_SEED):
    return synthetic_vgg_state_dict(seed)


def planar(img_u8, dtype):
    """uint8 [h][w][3] -> [1][3][h][w] in [0, 1]"""
    return torch.from_numpy(np.ascontiguousarray(img_u8)).permute(2, 0, 1)[None].to(dtype) / 255.0


# ---------------------------------------------------------------------------------------------------------- reference
def encode(x, sd, mutant=None):
    """x [1][3][h][w] -> [relu1_1, relu2_1, relu3_1, relu4_1], each [1][C][h][w], at x's dtype"""
    dt = x.dtype
    if mutant != "no 1x1 conv":
        x = F.conv2d(x, sd["0.weight"].to(dt), sd["0.bias"].to(dt))
    taps = []
    for idx, _, _ in VGG_CONVS[1:]:
        if idx > VGG_ENCODER_LAST:
            break
        x = F.pad(x, (1, 1, 1, 1), mode="constant" if mutant == "zero padding" else "reflect")
        x = F.relu(F.conv2d(x, sd[f"{idx}.weight"].to(dt), sd[f"{idx}.bias"].to(dt)))
        if idx in TAPS:
            taps.append(x)
        if idx in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2, 0, ceil_mode=mutant != "floor pooling")
    return taps


def mean_std(feat, mutant=None):
    """[1][C][h][w] -> (mean [C], std [C]) in fp64, whatever the map's dtype"""
    v = feat[0].reshape(feat.shape[1], -1).double()
    var = v.var(dim=1, unbiased=mutant != "biased variance") + (0.0 if mutant == "eps = 0" else EPS)
    return v.mean(dim=1), var if mutant == "std without sqrt" else var.sqrt()


def records(taps, mutant=None):
    """the four (mean, std) pairs as the device lays them out: float64 [1920]"""
    return torch.cat([torch.cat(mean_std(t, mutant)) for t in taps])


def loss_s_of(rec_a, rec_b):
    total = torch.zeros((), dtype=torch.float64)
    for o, c in zip(RECORD_OFFSETS, LEVEL_CHANNELS):
        total = total + ((rec_a[o:o + c] - rec_b[o:o + c]) ** 2).mean() + ((rec_a[o + c:o + 2 * c] - rec_b[o + c:o + 2 * c]) ** 2).mean()
    return total


def losses(frame, style, content, sd, dtype=torch.float64, mutant=None, enc=encode):
    """-> dict(loss_s, loss_c, rec) of uint8 images, the maps at `dtype`, the reductions in fp64"""
    with torch.no_grad():
        tf, ts, tc = (enc(planar(i, dtype), sd, mutant) for i in (frame, style, content))
        rec = records(tf, mutant)
        return {"loss_s": float(loss_s_of(rec, records(ts, mutant))),
                "loss_c": float(((tf[3].double() - tc[3].double()) ** 2).mean()), "rec": rec.numpy()}


def rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def group_errs(rec, want):
    """per record group (level x mean / std): max |err| / max |want|, eight figures"""
    out = []
    for o, c in zip(RECORD_OFFSETS, LEVEL_CHANNELS):
        for s in (o, o + c):
            g, w = np.asarray(rec[s:s + c], dtype=np.float64), np.asarray(want[s:s + c], dtype=np.float64)
            out.append(float(np.abs(g - w).max() / np.abs(w).max()))
    return out


def ratios(got, gold, case):
    """what FACTOR bounds: error / max(e32, FLOOR) of loss_s, loss_c and the eight record groups, against the golden fp64
    values, e32 the golden fp32 run's error under the same metric.  `got`: dict(loss_s[, loss_c][, rec])."""
    out = {}
    for key in ("loss_s", "loss_c"):
        if key in got and got[key] is not None:
            want = float(gold[f"{case}.{key}_f64"])
            out[key] = rel(got[key], want) / max(rel(float(gold[f"{case}.{key}_f32"]), want), FLOOR)
    if got.get("rec") is not None:
        e32 = group_errs(gold[f"{case}.rec_f32"], gold[f"{case}.rec_f64"])
        for i, (e, e3) in enumerate(zip(group_errs(got["rec"], gold[f"{case}.rec_f64"]), e32)):
            out[f"rec{i // 2 + 1}.{'std' if i % 2 else 'mean'}"] = e / max(e3, FLOOR)
    return out


# ------------------------------------------------------------------------------------------ the device's layout and route
def tokens(m):
    """[1][C][h][w] -> token-major [h*w][C]"""
    return m[0].reshape(m.shape[1], -1).t().contiguous()


def reflect_col(x, h, w):
    """token-major [h*w][C] -> the explicit column matrix [h*w][9 C] of a 3 x 3 conv under ReflectionPad2d(1), K order (ky, kx, c)"""
    c = x.shape[1]
    m = x.reshape(h, w, c)
    ry = np.abs(np.arange(-1, h + 1))
    ry = np.where(ry >= h, 2 * h - 2 - ry, ry)
    rx = np.abs(np.arange(-1, w + 1))
    rx = np.where(rx >= w, 2 * w - 2 - rx, rx)
    p = m[torch.from_numpy(ry)][:, torch.from_numpy(rx)]                  # [h+2][w+2][C]
    return torch.cat([p[ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], dim=2).reshape(h * w, 9 * c).contiguous()


def pack_weight(w):
    """[Cout][Cin][3][3] -> [Cout][9 Cinp] in K order (ky, kx, c), Cin padded to a multiple of 4 with zeros"""
    cout, cin = w.shape[:2]
    p = w.permute(0, 2, 3, 1)
    if cin % 4:
        p = F.pad(p, (0, 4 - cin % 4))
    return p.reshape(cout, -1).contiguous()


def input_f32(x3, a, b):
    """numpy float32 statement of the input kernels: x3 [n][3] float32 (already / 255), a [3][3], b [3] -> [n][4]"""
    f = np.float32
    x3, a, b = x3.astype(f), a.astype(f), b.astype(f)
    out = np.zeros((x3.shape[0], 4), f)
    for o in range(3):
        out[:, o] = ((a[o, 0] * x3[:, 0] + a[o, 1] * x3[:, 1]).astype(f) + (a[o, 2] * x3[:, 2]).astype(f)).astype(f) + b[o]
    return out


def encode_restated(x, sd, mutant=None):
    """encode() as the device computes it, in fp32: fixed-order input conv, six-product split GEMMs, exact pools"""
    assert mutant is None
    h, w = x.shape[2:]
    img = x[0].reshape(3, -1).t().numpy().astype(np.float32)
    cur = torch.from_numpy(input_f32(img, sd["0.weight"].reshape(3, 3).numpy(), sd["0.bias"].numpy()))
    taps = []
    for idx, _, cout in VGG_CONVS[1:]:
        if idx > VGG_ENCODER_LAST:
            break
        y = O.gemm_restated(reflect_col(cur, h, w), pack_weight(sd[f"{idx}.weight"]), sd[f"{idx}.bias"])
        cur = F.relu(y)
        if idx in TAPS:
            taps.append(cur.t().reshape(1, cout, h, w))
        if idx in POOL_AFTER:
            cur = tokens(F.max_pool2d(cur.t().reshape(1, cout, h, w), 2, 2, 0, ceil_mode=True))
            h, w = (h + 1) // 2, (w + 1) // 2
    return taps
