"""The masked interpolation as a composition of two functions the oracle already pins to the reference (tests/test_oracle.py):
per sample and label, ``cpu_ref.interpolation`` (models/cWCT.py:206-262) on the gathered columns as a batch of one, for the labels
that pass ``cpu_ref.compute_label_info`` (:166-189) against EVERY style map; other pixels keep the content feature."""
import numpy as np
import torch

from oracle import cpu_ref


def interpolation_seg_ref(content, styles, alphas, alpha_c, cmask, smasks, use_double=False, interp=None):
    """content [B,N,H,W], styles = list of [B,N,h,w], cmask[b], smasks[i][b] label maps.  `interp` replaces
    cpu_ref.interpolation (the fixture's generator passes the reference's own method)."""
    interp = interp or (lambda c, ss, a, ac: cpu_ref.interpolation(c, ss, a, ac, use_double=use_double))
    B, N = content.shape[:2]
    out = content.clone().reshape(B, N, -1)
    for b in range(B):
        infos = [cpu_ref.compute_label_info(cmask[b], sm[b]) for sm in smasks]
        cm = torch.from_numpy(np.asarray(cmask[b]).reshape(-1).astype(np.int64))
        for l in infos[0][0]:
            if not all(ok[l] for _, ok in infos):
                continue
            ci = torch.nonzero(cm == int(l)).reshape(-1)
            cols = content[b].reshape(N, -1)[:, ci][None, :, :, None]
            scols = []
            for s, sm in zip(styles, smasks):
                si = torch.nonzero(torch.from_numpy(np.asarray(sm[b]).reshape(-1).astype(np.int64)) == int(l)).reshape(-1)
                scols.append(s[b].reshape(N, -1)[:, si][None, :, :, None])
            out[b][:, ci] = interp(cols, scols, list(alphas), alpha_c)[0, :, :, 0].to(out.dtype)
    return out.reshape(content.shape)


def region_mask(h, w, labels, seed, tiny=None):
    """uint8 [h,w]: vertical bands of `labels` (a list) with a wavy edge; `tiny` = a label put on 6 pixels only."""
    rng = np.random.default_rng(seed)
    edges = np.linspace(0, w, len(labels) + 1)
    m = np.zeros((h, w), dtype=np.uint8)
    for y in range(h):
        shift = rng.integers(-2, 3)
        for k, l in enumerate(labels):
            a = 0 if k == 0 else int(edges[k]) + shift
            m[y, max(a, 0):] = l
    if tiny is not None:
        m[1:3, 1:4] = tiny
    return m
