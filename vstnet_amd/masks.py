"""Mask producers on the device (csrc/masks.hip): what a per-frame label map needs before the masked transfer.

The reference's video loop segments every frame and post-processes its label map (video_transfer.py:161-186:
``self_remapping``, ``cross_remapping``, then ``cwct.transfer`` with that frame's ``content_seg``).  Here a map is uploaded
once and everything after that is stream-ordered device work: colours to labels, histogram, the remapping as a 256-entry
table, the label plan.  The remapped map itself is never written: the masked kernels read ``plan.lut[raw label]``.

This module also holds the numpy MODEL of the small kernels (``remap_lut_model``, ``plan_model``): their specification, checked
against ``models.segmentation.SegReMapping`` on the host (tests/test_masks_host.py) and against the kernels on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

OVERFLOW = _lib.MASK_OVERFLOW
OUT_OF_TABLE = _lib.MASK_OUT_OF_TABLE
PACKED_SLOTS = 8            # slots of the packed masked route (cWCT.ROUTES["masked_packed_rows"])
MAX_SLOTS = 32


# ---------------------------------------------------------------------------------------------- host side: threshold + model
def min_count(n_pixels, min_ratio):
    """Smallest pixel count whose share passes ``SegReMapping.self_remapping``'s test, found with the class's OWN expression
    (``np.float32(count) / n_pixels < min_ratio``; monotone in count): the device compares integers against it and so decides
    exactly like the host at the boundary.  0 when every count passes."""
    n_pixels = int(n_pixels)
    below = lambda c: bool(np.float32(c) / n_pixels < min_ratio)      # noqa: E731
    if not below(0):
        return 0
    lo, hi = 0, n_pixels + 1          # below(lo); hi: first count known (or assumed) to pass
    if below(n_pixels):
        return n_pixels + 1           # (min_ratio > 1: nothing passes)
    hi = n_pixels
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if below(mid):
            lo = mid
        else:
            hi = mid
    return hi


def remap_lut_model(hist, table, threshold=0, style_hist=None):
    """vst_remap_lut in numpy: (lut uint8[256], histogram of the remapped map int64[256], flags)."""
    hist = np.asarray(hist, dtype=np.int64)
    table = np.asarray(table)
    rows, cols = table.shape
    flags = 0

    def related(l, ok):
        nonlocal flags
        if l >= cols:
            flags |= OUT_OF_TABLE
            return l
        for j in range(rows):
            cand = int(table[j, l])
            if 0 <= cand < 256 and ok(cand):
                return cand
        return l

    self_lut = np.arange(256)
    for l in range(256):
        if 0 < hist[l] < threshold:
            self_lut[l] = related(l, lambda c: hist[c] > 0 and hist[c] >= threshold)
    h1 = np.zeros(256, np.int64)
    np.add.at(h1, self_lut, hist)
    cross_lut = np.arange(256)
    if style_hist is not None:
        sh = np.asarray(style_hist, dtype=np.int64)
        for l in range(256):
            if h1[l] > 0 and sh[l] <= 0:
                cross_lut[l] = related(l, lambda c: sh[c] > 0)
    h2 = np.zeros(256, np.int64)
    np.add.at(h2, cross_lut, h1)
    lut = np.where(hist > 0, cross_lut[self_lut], np.arange(256)).astype(np.uint8)
    return lut, h2, flags


def plan_model(hist_c, remap, hist_s, cap):
    """vst_label_plan_hist in numpy: (n_slots, overflow, lut uint8[256] raw label -> slot (255 = none), slot_label list)."""
    hist_c = np.asarray(hist_c, dtype=np.int64)
    hist_s = np.asarray(hist_s, dtype=np.int64)
    remap = np.arange(256) if remap is None else np.asarray(remap).astype(np.int64)
    hc = np.zeros(256, np.int64)
    np.add.at(hc, remap, hist_c)
    slot_of = np.full(256, 255, np.uint8)
    slot_label, over = [], False
    for l in range(256):
        a, b = int(hc[l]), int(hist_s[l])
        if a > 10 and b > 10 and a / b < 100 and b / a < 100:
            if len(slot_label) < cap:
                slot_of[l] = len(slot_label)
                slot_label.append(l)
            else:
                over = True
    return len(slot_label), over, slot_of[remap], slot_label


# ---------------------------------------------------------------------------------------------- device side
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u8_device(t, what):
    import torch
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8:
        raise ValueError(f"{what} must be a uint8 tensor on the GPU (no CPU fallback)")
    return t.contiguous()


def colors_to_labels(rgb_dev):
    """uint8 [H,W,3] colour map on the device -> uint8 [H,W] labels (utils.colors_to_labels, bit-exact)."""
    import torch
    rgb = _u8_device(rgb_dev, "rgb_dev")
    if rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected [H,W,3], got {tuple(rgb.shape)}")
    out = torch.empty(rgb.shape[:2], dtype=torch.uint8, device=rgb.device)
    with torch.cuda.device(rgb.device):
        _lib.check(_lib.lib().vst_colors_to_labels(_ptr(rgb), _ptr(out), out.numel(), _stream()), "vst_colors_to_labels")
    return out


def label_hist(labels_dev, out=None):
    """int32 [256] histogram of a uint8 label map on the device."""
    import torch
    m = _u8_device(labels_dev, "labels_dev")
    if out is None:
        out = torch.empty(256, dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        _lib.check(_lib.lib().vst_label_hist(_ptr(m), m.numel(), _ptr(out), _stream()), "vst_label_hist")
    return out


def apply_lut(labels_dev, lut_dev):
    import torch
    m = _u8_device(labels_dev, "labels_dev")
    out = torch.empty_like(m)
    with torch.cuda.device(m.device):
        _lib.check(_lib.lib().vst_apply_lut(_ptr(m), _ptr(lut_dev), _ptr(out), m.numel(), _stream()), "vst_apply_lut")
    return out


class DeviceSegReMapping:
    """``models.segmentation.SegReMapping`` on uint8 device tensors: same constructor, same two methods, same results.  The
    relation table lives on the device as int16 (uploaded on first use per device); every call is one histogram, one
    single-workgroup launch that builds the 256-entry table, and one gather - no host synchronisation.  A label that needs the
    table but lies outside it raises ``OUT_OF_TABLE`` in ``self.flags`` (the host class raises IndexError there);
    ``check()`` reads the word back."""

    def __init__(self, mapping, min_ratio=0.01):
        table = np.load(mapping) if isinstance(mapping, (str, bytes)) else np.asarray(mapping)
        if table.ndim != 2:
            raise ValueError(f"the relation table must be [rows, cols], got {table.shape}")
        if table.min() < -32768 or table.max() > 32767:
            raise ValueError("relation table entries must fit int16")
        self.table = np.ascontiguousarray(table.astype(np.int16))
        self.min_ratio = min_ratio
        self._dev = {}
        self._thresholds = {}
        self.flags = None

    @property
    def shape(self):
        return self.table.shape

    def threshold(self, n_pixels):
        t = self._thresholds.get(n_pixels)
        if t is None:
            t = self._thresholds[n_pixels] = min_count(n_pixels, self.min_ratio)
        return t

    def table_on(self, device):
        import torch
        key = str(device)
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = (torch.from_numpy(self.table).to(device), torch.zeros(1, dtype=torch.int32, device=device))
        self.flags = t[1]
        return t[0]

    def lut(self, hist, n_pixels, style_hist=None, self_remap=True, out=None, hist_out=None, flags=None):
        """The composed table for a map with histogram `hist` (device int32[256]): uint8 [256] on the device."""
        import torch
        table = self.table_on(hist.device)
        if out is None:
            out = torch.empty(256, dtype=torch.uint8, device=hist.device)
        rows, cols = self.table.shape
        with torch.cuda.device(hist.device):
            _lib.check(_lib.lib().vst_remap_lut(_ptr(hist), _ptr(style_hist), _ptr(table), rows, cols,
                                                self.threshold(int(n_pixels)) if self_remap else 0, _ptr(out), _ptr(hist_out),
                                                _ptr(flags if flags is not None else self.flags), _stream()), "vst_remap_lut")
        return out

    def self_remapping(self, seg):
        seg = _u8_device(seg, "seg")
        return apply_lut(seg, self.lut(label_hist(seg), seg.numel()))

    def cross_remapping(self, content_seg, style_seg):
        c, s = _u8_device(content_seg, "content_seg"), _u8_device(style_seg, "style_seg")
        return apply_lut(c, self.lut(label_hist(c), c.numel(), style_hist=label_hist(s), self_remap=False))

    def check(self):
        """Raise like the host class if any call so far met a label outside the table (synchronises)."""
        if self.flags is not None and int(self.flags.item()) & OUT_OF_TABLE:
            raise IndexError("a label that needs the relation table lies outside it")
