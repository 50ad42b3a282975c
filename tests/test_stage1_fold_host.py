"""The index maps of the tap-folded 16 -> 4 conv (csrc/conv.hip, conv_mfma_kernel<..., FOLD>) restated on the CPU: the folded weight
operand is a gather of 16-byte items of the packed fragment block (csrc/layout.hip, pack_conv_kernel: the packed layout and
vst_conv_packed_bytes do not change), the pixel operand is the staged image read un-shifted over a wave's linearised 4 x 18
region, and the shift-add of the three partial sums gives the 3 x 3 reflect-padded convolution.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from vstnet_amd import _lib

CIN, COUT, IW, MR, NSLOT = 16, 4, 18, 4, 336


def packed_items(w):
    """pack_conv_kernel's fragment block for cin = 16: item (ks, kg, co) = 8 values over j: tap = 2 ks + (kg >> 1), ci = 8 (kg & 1) + j"""
    items = np.zeros((5, 4, 16, 8))
    for ks in range(5):
        for kg in range(4):
            tap = 2 * ks + (kg >> 1)
            for co in range(COUT):
                if tap < 9:
                    items[ks, kg, co] = w[co, 8 * (kg & 1):8 * (kg & 1) + 8, tap // 3, tap % 3]
    return items


def folded_items(items):
    """the kernel's staging gather: folded item (r = 4 ks + kg, row = 4 tx + co) <- packed item of tap 3 ty + tx, or zero"""
    out = np.zeros((8, 16, 8))
    for r in range(8):
        for row in range(16):
            ty, tx = 2 * (r >> 2) + ((r >> 1) & 1), row >> 2
            if ty < 3 and tx < 3:
                tap = 3 * ty + tx
                out[r, row] = items[tap >> 1, (tap & 1) * 2 + (r & 1), row & 3]
    return out


def test_packed_bytes_unchanged():
    """the folded form reads the existing fragment block: the size the host test of the layout pins stays what it was"""
    L = _lib.lib()
    assert L.vst_conv_packed_bytes(4, 16) == ((9 * 16 * 4 * 4 + 255) // 256 * 256) + 3 * (5 * 4 * 16 * 16)


def test_fold_index_map_is_the_convolution():
    rng = np.random.default_rng(0)
    w = rng.standard_normal((COUT, CIN, 3, 3))
    x = rng.standard_normal((CIN, 16, 16))
    fold = folded_items(packed_items(w))
    # every weight appears exactly once, everything else is zero
    assert np.count_nonzero(fold) == w.size and np.isclose(np.abs(fold).sum(), np.abs(w).sum())
    # the staged image of one 16 x 16 tile: [channel group][slot = iy * 18 + ix][8]
    xp = F.pad(torch.from_numpy(x)[None], (1, 1, 1, 1), mode="reflect")[0].numpy()       # 16 x 18 x 18
    img = np.zeros((2, NSLOT, 8))
    for cig in range(2):
        img[cig, :IW * IW] = xp[8 * cig:8 * cig + 8].reshape(8, -1).T
    out = np.zeros((COUT, 16, 16))
    for wave in range(4):
        D = np.zeros((16, 80))                       # [row = 4 tx + co][q]
        for ks in range(2):
            for kg in range(4):
                ty = min(2 * ks + (kg >> 1), 2)
                for q in range(80):
                    qq = min(q, MR * IW - 1)
                    b = img[kg & 1, (wave * MR + ty) * IW + qq]              # the lane's 8 K values of pixel q
                    D[:, q] += fold[4 * ks + kg] @ b
        for r in range(MR):
            for xo in range(16):
                q0 = r * IW + xo
                for co in range(COUT):
                    out[co, wave * MR + r, xo] = (D[co, q0] + D[4 + co, q0 + 1]) + D[8 + co, q0 + 2]
    ref = F.conv2d(torch.from_numpy(xp)[None], torch.from_numpy(w))[0].numpy()
    assert np.allclose(out, ref, rtol=0, atol=1e-12)
