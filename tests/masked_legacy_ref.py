"""The one-style masked transfer composed WITHOUT the driver's plan builder and factor call, as a third side for the
bit-identity tests of tests/test_gpu_masked_interp.py (the driver computes the masked transfer as the one-style interpolation, so
`transfer` vs `interpolation` alone would compare a path with itself):

  * from the library's single-style entry points, called through ctypes: vst_label_plan, vst_label_plan_hist,
    vst_cwct_stats_labels / _labels_code, vst_cwct_factor_labels / _keyed, vst_cwct_apply_labels;
  * per label, from the public cWCT.stats / factor / apply over compute_label_info's valid labels (models/cWCT.py:83-103);
  * the plan table in numpy (vstnet_amd.masks.plan_model), which depends on neither C entry point.
"""
import ctypes as C

import numpy as np
import torch

from vstnet_amd import _lib, masks

SLOTS = 32
EPS = 2e-5


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8))).cuda().reshape(-1)


def empty(n, dtype):
    return torch.empty(n, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ plan tables
def table_fields(table):
    """The six fields of a 2344-byte label plan (csrc/common.h LabelPlan) as host arrays."""
    raw = table.cpu().numpy()
    assert raw.size == _lib.LABEL_PLAN_BYTES
    i32 = lambda a, b: raw[a:b].view(np.int32)      # noqa: E731
    return {"n_slots": int(i32(0, 4)[0]), "overflow": int(i32(4, 8)[0]), "hist_c": i32(8, 1032), "hist_s": i32(1032, 2056),
            "lut": raw[2056:2312], "slot_label": raw[2312:2344]}


def assert_table_is_the_numpy_plan(table, cm, sms, cap=SLOTS, content_lut=None):
    """Every byte of `table` from numpy alone: histograms by bincount, validity and slots by masks.plan_model, once per style map
    (a label needs a slot against every one)."""
    f = table_fields(table)
    hc = np.bincount(np.asarray(cm).reshape(-1), minlength=256)
    hs = [np.bincount(np.asarray(m).reshape(-1), minlength=256) for m in sms]
    valid = None
    for h in hs:
        _, _, _, labels = masks.plan_model(hc, content_lut, h, 256)
        valid = set(labels) if valid is None else valid & set(labels)
    labels = sorted(valid)
    lut = np.full(256, 255, np.uint8)
    for k, l in enumerate(labels[:cap]):
        lut[l] = k
    assert f["n_slots"] == min(len(labels), cap) and f["overflow"] == int(len(labels) > cap)
    assert np.array_equal(f["hist_c"], hc) and np.array_equal(f["hist_s"], np.min(hs, axis=0))
    assert np.array_equal(f["lut"], lut)
    assert np.array_equal(f["slot_label"], np.array(labels[:cap] + [0] * (SLOTS - min(len(labels), cap)), np.uint8))
    return labels[:cap]


def legacy_plan(cm_dev, sm_dev):
    """vst_label_plan of two flat uint8 device maps."""
    tab = empty(_lib.LABEL_PLAN_BYTES, torch.uint8)
    _lib.check(_lib.lib().vst_label_plan(ptr(cm_dev), cm_dev.numel(), ptr(sm_dev), sm_dev.numel(), ptr(tab), stream()), "vst_label_plan")
    return tab


# ------------------------------------------------------------------------------------------------ the legacy calls
def stats_labels(x2d, mask, table, max_slots):
    L = _lib.lib()
    N, Lp = x2d.shape
    out = empty(SLOTS * (1 + N + N * N), torch.float64)
    ws = empty(max(1, L.vst_cwct_labels_workspace_bytes(N, Lp)), torch.uint8)
    _lib.check(L.vst_cwct_stats_labels(ptr(x2d), N, Lp, ptr(mask), ptr(table), max_slots, ptr(out), ptr(ws), stream()),
               "vst_cwct_stats_labels")
    return out


def stats_labels_code(rows, H, W, mask_rows, table, max_slots):
    L = _lib.lib()
    out = empty(SLOTS * (1 + 32 + 32 * 32), torch.float64)
    ws = empty(max(1, L.vst_cwct_stats_labels_code_workspace_bytes(H, W)), torch.uint8)
    _lib.check(L.vst_cwct_stats_labels_code(ptr(rows), H, W, ptr(mask_rows), ptr(table), max_slots, ptr(out), ptr(ws), stream()),
               "vst_cwct_stats_labels_code")
    return out


def factor_labels(cs, ss, table, max_slots, N, style_plan=None):
    """vst_cwct_factor_labels, or with a style plan vst_cwct_factor_labels_keyed -> affines [32 * (N*N + N)]."""
    L = _lib.lib()
    aff, info = empty(SLOTS * (N * N + N), torch.float32), empty(SLOTS * 3, torch.int32)
    if style_plan is None:
        _lib.check(L.vst_cwct_factor_labels(ptr(cs), ptr(ss), ptr(table), max_slots, EPS, N, ptr(aff), ptr(info), stream()),
                   "vst_cwct_factor_labels")
    else:
        _lib.check(L.vst_cwct_factor_labels_keyed(ptr(cs), ptr(ss), ptr(table), ptr(style_plan), max_slots, EPS, N, ptr(aff),
                                                  ptr(info), stream()), "vst_cwct_factor_labels_keyed")
    return aff


def apply_labels(x2d, aff, mask, table, max_slots, precision):
    N, Lp = x2d.shape
    out = torch.empty_like(x2d)
    _lib.check(_lib.lib().vst_cwct_apply_labels(ptr(x2d), ptr(out), N, Lp, ptr(aff), ptr(mask), ptr(table), max_slots,
                                                _lib.PRECISIONS[precision], stream()), "vst_cwct_apply_labels")
    return out


def mask_rows(mask, H, W):
    rows = torch.empty_like(mask)
    _lib.check(_lib.lib().vst_mask_to_code(ptr(mask), ptr(rows), H, W, stream()), "vst_mask_to_code")
    return rows


# ------------------------------------------------------------------------------------------------ composed transfers
def transfer_single_pass(c, s, cm, sm, precision):
    """masked_single_pass by hand: per sample vst_label_plan, the statistics of both codes, vst_cwct_factor_labels and
    vst_cwct_apply_labels, all slots (max_slots = 0) -> (output, tables, affines)."""
    B, N = c.shape[:2]
    c2, s2 = c.float().contiguous().reshape(B, N, -1), s.float().contiguous().reshape(B, N, -1)
    out, tables, affines = torch.empty_like(c2), [], []
    for b in range(B):
        cmd, smd = dev_u8(cm[b]), dev_u8(sm[b])
        tab = legacy_plan(cmd, smd)
        aff = factor_labels(stats_labels(c2[b], cmd, tab, 0), stats_labels(s2[b], smd, tab, 0), tab, 0, N)
        out[b] = apply_labels(c2[b], aff, cmd, tab, 0, precision)
        tables.append(tab)
        affines.append(aff)
    return out.reshape(c.shape), tables, affines


def transfer_packed_rows(z, s, cm, sm, max_slots):
    """masked_packed_rows by hand on a PackedCode: vst_label_plan, vst_cwct_stats_labels_code on the rows with the map in the
    rows' order, vst_cwct_stats_labels on the style, vst_cwct_factor_labels; the maps attached as pending (vstnet_amd/code.py
    applies them) -> (PackedCode, tables, affines)."""
    B, N, H, W = z.shape
    s2 = s.float().contiguous().reshape(B, N, -1)
    per_image, tables, affines = [], [], []
    for b in range(B):
        cmd, smd = dev_u8(cm[b]), dev_u8(sm[b])
        tab = legacy_plan(cmd, smd)
        rows = mask_rows(cmd, H, W)
        aff = factor_labels(stats_labels_code(z.packed[b], H, W, rows, tab, max_slots), stats_labels(s2[b], smd, tab, max_slots),
                            tab, max_slots, N)
        per_image.append((aff, rows, tab))
        tables.append(tab)
        affines.append(aff)
    return z.with_label_affines(per_image, max_slots), tables, affines


def transfer_per_label(cw, c, s, cm, sm):
    """The reference's loop (models/cWCT.py:83-103) from the public per-matrix calls: for every label compute_label_info keeps,
    statistics of the label's columns in both codes, one factor, one apply under the content map."""
    B, N = c.shape[:2]
    c2, s2 = c.float().contiguous().reshape(B, N, -1), s.float().contiguous().reshape(B, N, -1)
    out = c2.clone()
    for b in range(B):
        label_set, indicator = cw.compute_label_info(cm[b], sm[b])
        cmd, smd = dev_u8(cm[b]), dev_u8(sm[b])
        for label in label_set:
            if indicator[label]:
                affine = cw.factor(cw.stats(c2[b], cmd, int(label)), [cw.stats(s2[b], smd, int(label))], [1.0], 0.0, N)
                cw.apply(c2[b], affine, out=out[b], mask=cmd, label=int(label))
    return out.reshape(c.shape).to(c.dtype)


def transfer_keyed_frame(z, s, cm, sm, cap, precision):
    """The per-frame transfer of ONE image by hand.  Style side keyed by label: histogram of the style map, its plan against
    itself (vst_label_plan_hist), per-slot statistics, prefactored.  Frame: histogram (fused with the row order for the packed
    route), vst_label_plan_hist with cap `cap`, statistics, vst_cwct_factor_labels_keyed, then the dense apply (cap 32) or the
    pending per-row maps (cap 8, `z` a PackedCode) -> (output, table, affines)."""
    L = _lib.lib()
    N, H, W = z.shape[1:]
    s2 = s.float().contiguous().reshape(N, -1)
    cmd, smd = dev_u8(cm), dev_u8(sm)
    hist_s, plan_s = empty(256, torch.int32), empty(_lib.LABEL_PLAN_BYTES, torch.uint8)
    _lib.check(L.vst_label_hist(ptr(smd), smd.numel(), ptr(hist_s), stream()), "vst_label_hist")
    _lib.check(L.vst_label_plan_hist(ptr(hist_s), None, ptr(hist_s), SLOTS, ptr(plan_s), None, stream()), "vst_label_plan_hist")
    ss = stats_labels(s2, smd, plan_s, 0)
    pinfo = empty(SLOTS, torch.int32)
    _lib.check(L.vst_cwct_prefactor_labels(ptr(ss), ptr(plan_s), 0, N, EPS, ptr(ss), ptr(pinfo), stream()), "vst_cwct_prefactor_labels")
    hist_c, tab, rows = empty(256, torch.int32), empty(_lib.LABEL_PLAN_BYTES, torch.uint8), empty(H * W, torch.uint8)
    if cap <= 8:
        _lib.check(L.vst_mask_prepare(ptr(cmd), 0, H, W, ptr(rows), ptr(hist_c), stream()), "vst_mask_prepare")
    else:
        _lib.check(L.vst_label_hist(ptr(cmd), cmd.numel(), ptr(hist_c), stream()), "vst_label_hist")
    _lib.check(L.vst_label_plan_hist(ptr(hist_c), None, ptr(hist_s), cap, ptr(tab), None, stream()), "vst_label_plan_hist")
    if cap <= 8:
        aff = factor_labels(stats_labels_code(z.packed[0], H, W, rows, tab, cap), ss, tab, cap, N, style_plan=plan_s)
        return z.with_label_affines([(aff, rows, tab)], cap), tab, aff
    c2 = z.float().contiguous().reshape(N, -1)
    aff = factor_labels(stats_labels(c2, cmd, tab, cap), ss, tab, cap, N, style_plan=plan_s)
    return apply_labels(c2, aff, cmd, tab, cap, precision).reshape(z.shape), tab, aff
