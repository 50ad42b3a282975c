"""The cWCT kernels one by one (``vstnet_amd.cwct.ops``): thin wrappers of the cWCT calls of include/vstnet.h, one launch or one
launcher call each, for tests and tools.

Unlike ``vstnet_amd.segformer.ops`` these take contiguous views at ANY element offset: in csrc/cwct.hip alignment is a launch
condition (it picks the kernel form), not a requirement.  Only dtype, device, contiguity and shape are checked here.  Dense
features are x [N, L] float32; statistics records double [1 + N + N*N] (``{n, mean, cov}``), per-slot blocks double
[32, 1 + N + N*N]; affines float32 [N*N + N] (``{T, t0}``), per-slot [32, N*N + N]; a plan is a uint8 [LABEL_PLAN_BYTES] buffer.
Workspaces are sized with the library's ``*_workspace_bytes`` calls.  Everything is queued on torch's current stream; the
library refuses what it cannot run (``VstError``); there is no torch implementation behind any of these.
"""
from __future__ import annotations

import ctypes as C

from . import _lib

MAX_SLOTS = 32
PLAN_N_SLOTS, PLAN_LUT, PLAN_SLOT_LABEL = 0, 8 + 2 * 256 * 4, 8 + 2 * 256 * 4 + 256     # byte offsets inside a plan record


def _t(name, t, dtype, shape=None):
    """dtype, contiguity and shape; the device is checked where the pointer is taken (_ptr), after every argument's shape, so
    that all refusals answer on a machine without a GPU"""
    import torch
    what = str(dtype).replace("torch.", "")
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError(f"{name} must be a {what} tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (a view at any element offset is fine)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _f32(name, t, shape=None):
    import torch
    return _t(name, t, torch.float32, shape)


def _f64(name, t, shape=None):
    import torch
    return _t(name, t, torch.float64, shape)


def _u8(name, t, shape=None):
    import torch
    return _t(name, t, torch.uint8, shape)


def _x2d(name, x):
    import torch
    if torch.is_tensor(x) and x.dim() != 2:
        raise ValueError(f"{name} must be [N, L], got shape {tuple(x.shape)}")
    return _f32(name, x).shape


def _cuda(t):
    if t is not None and not t.is_cuda:
        raise ValueError("every tensor must be a CUDA tensor")
    return t


def _ptr(t):
    return C.c_void_p(_cuda(t).data_ptr() if t is not None else 0)


def _call(name, like, *args):
    import torch
    with torch.cuda.device(like.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(getattr(_lib.lib(), name)(*args, st), name)


def _workspace(nbytes, like):
    import torch
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


def _rec(n):
    return 1 + n + n * n


def _prec(precision):
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}")
    return _lib.PRECISIONS[precision]


def _out_like(out, x, name="out"):
    import torch
    if out is None:
        return torch.empty_like(x)
    return _f32(name, out, x.shape)


def _host_ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[_cuda(t).data_ptr() if t is not None else 0 for t in tensors])


# ---------------------------------------------------------------------------------------------------------- one pair
def stats(x, mask=None, label=0, out=None):
    """{n, mean, cov} of x [N, L] over all pixels, or over those with mask [L] == label (vst_cwct_stats)."""
    import torch
    n, l = _x2d("x", x)
    if mask is not None:
        _u8("mask", mask, (l,))
    out = torch.empty(_rec(n), dtype=torch.float64, device=x.device) if out is None else _f64("out", out, (_rec(n),))
    ws = _workspace(_lib.lib().vst_cwct_stats_workspace_bytes(n, l), x)
    _call("vst_cwct_stats", x, _ptr(x), n, l, _ptr(mask), int(label), _ptr(out), _ptr(ws))
    return out


def factor(content, styles, alphas, n, alpha_c=0.0, eps=2e-5, min_tries=None, affine=None):
    """(affine [N*N + N], info [2 + n_styles]) of one content record against 1..8 style records (vst_cwct_factor).
    ``min_tries``: the IN side of info (retries to start from), zeros when None."""
    import torch
    _f64("content", content, (_rec(n),))
    if not 1 <= len(styles) <= _lib.MAX_STYLES or len(alphas) != len(styles):
        raise ValueError(f"factor takes 1..{_lib.MAX_STYLES} styles and as many alphas")
    for s in styles:
        _f64("style", s, (_rec(n),))
    k = len(styles)
    info = torch.zeros(2 + k, dtype=torch.int32, device=content.device)
    if min_tries is not None:
        info.copy_(torch.as_tensor(list(min_tries), dtype=torch.int32))
    affine = torch.empty(n * n + n, dtype=torch.float32, device=content.device) if affine is None else _f32("affine", affine, (n * n + n,))
    al = (C.c_float * k)(*[float(a) for a in alphas])
    _call("vst_cwct_factor", content, _ptr(content), _host_ptrs(styles), al, k, float(alpha_c), float(eps), n, _ptr(affine),
          _ptr(info))
    return affine, info


def prefactor(rec, n, eps=2e-5, out=None):
    """(prefactored record {-(n+1), mean, chol(cov)}, info [1] retries) (vst_cwct_prefactor); ``out`` may be ``rec``."""
    import torch
    _f64("rec", rec, (_rec(n),))
    out = torch.empty_like(rec) if out is None else _f64("out", out, (_rec(n),))
    info = torch.zeros(1, dtype=torch.int32, device=rec.device)
    _call("vst_cwct_prefactor", rec, _ptr(rec), n, float(eps), _ptr(out), _ptr(info))
    return out, info


def apply(x, affine, out=None, mask=None, label=0, precision="bf16x3"):
    """out[:, p] = T x[:, p] + t0 (vst_cwct_apply_prec); with a mask only pixels of ``label`` are written; ``out`` may be ``x``."""
    n, l = _x2d("x", x)
    _f32("affine", affine, (n * n + n,))
    if mask is not None:
        _u8("mask", mask, (l,))
    out = _out_like(out, x)
    _call("vst_cwct_apply_prec", x, _ptr(x), _ptr(out), n, l, _ptr(affine), _ptr(mask), int(label), _prec(precision))
    return out


# ------------------------------------------------------------------------------------------------------------ labels
def label_plan(cmask, smask, plan=None):
    """plan record of two uint8 label maps (vst_label_plan)."""
    import torch
    _u8("cmask", cmask), _u8("smask", smask)
    plan = torch.empty(_lib.LABEL_PLAN_BYTES, dtype=torch.uint8, device=cmask.device) if plan is None else \
        _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    _call("vst_label_plan", cmask, _ptr(cmask), cmask.numel(), _ptr(smask), smask.numel(), _ptr(plan))
    return plan


def plan_info(plan):
    """(n_slots, overflow, lut [256], slot_label [32]) of a plan, on the host (synchronises)."""
    import numpy as np
    b = _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,)).cpu().numpy()
    head = b[:8].view(np.int32)
    return int(head[0]), int(head[1]), b[PLAN_LUT:PLAN_LUT + 256].copy(), b[PLAN_SLOT_LABEL:PLAN_SLOT_LABEL + MAX_SLOTS].copy()


def _slots(max_slots):
    if not 0 <= int(max_slots) <= MAX_SLOTS:
        raise ValueError(f"max_slots must be 0..{MAX_SLOTS}")
    return int(max_slots)


def stats_labels(x, mask, plan, max_slots=0, out=None):
    """records [32, 1 + N + N*N] of every slot of ``plan`` in one launcher call (vst_cwct_stats_labels); N in {32, 64, 128}."""
    import torch
    n, l = _x2d("x", x)
    _u8("mask", mask, (l,)), _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    out = torch.empty((MAX_SLOTS, _rec(n)), dtype=torch.float64, device=x.device) if out is None else \
        _f64("out", out, (MAX_SLOTS, _rec(n)))
    ws = _workspace(_lib.lib().vst_cwct_labels_workspace_bytes(n, l), x)
    _call("vst_cwct_stats_labels", x, _ptr(x), n, l, _ptr(mask), _ptr(plan), _slots(max_slots), _ptr(out), _ptr(ws))
    return out


def _affines(affines, n, like):
    import torch
    if affines is None:
        return torch.empty((MAX_SLOTS, n * n + n), dtype=torch.float32, device=like.device)
    return _f32("affines", affines, (MAX_SLOTS, n * n + n))


def factor_labels(content, style, plan, n, eps=2e-5, max_slots=0, style_plan=None, affines=None):
    """(affines [32, N*N + N], info [32, 3]): vst_cwct_factor_labels, or with ``style_plan`` vst_cwct_factor_labels_keyed."""
    import torch
    _f64("content", content, (MAX_SLOTS, _rec(n))), _f64("style", style, (MAX_SLOTS, _rec(n)))
    _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    affines = _affines(affines, n, content)
    info = torch.zeros((MAX_SLOTS, 3), dtype=torch.int32, device=content.device)
    if style_plan is None:
        _call("vst_cwct_factor_labels", content, _ptr(content), _ptr(style), _ptr(plan), _slots(max_slots), float(eps), n,
              _ptr(affines), _ptr(info))
    else:
        _u8("style_plan", style_plan, (_lib.LABEL_PLAN_BYTES,))
        _call("vst_cwct_factor_labels_keyed", content, _ptr(content), _ptr(style), _ptr(plan), _ptr(style_plan),
              _slots(max_slots), float(eps), n, _ptr(affines), _ptr(info))
    return affines, info


def factor_labels_mix(content, styles, alphas, plan, n, alpha_c=0.0, eps=2e-5, max_slots=0, style_plans=None, affines=None):
    """(affines, info [32, 2 + n_styles]) of 1..8 per-slot style blocks (vst_cwct_factor_labels_mix); ``style_plans``: None, or one
    plan or None per style."""
    import torch
    _f64("content", content, (MAX_SLOTS, _rec(n))), _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    k = len(styles)
    if not 1 <= k <= _lib.MAX_STYLES or len(alphas) != k or (style_plans is not None and len(style_plans) != k):
        raise ValueError(f"factor_labels_mix takes 1..{_lib.MAX_STYLES} styles, as many alphas and (optionally) as many plans")
    for s in styles:
        _f64("style", s, (MAX_SLOTS, _rec(n)))
    for p in style_plans or ():
        if p is not None:
            _u8("style_plan", p, (_lib.LABEL_PLAN_BYTES,))
    affines = _affines(affines, n, content)
    info = torch.zeros((MAX_SLOTS, 2 + k), dtype=torch.int32, device=content.device)
    al = (C.c_float * k)(*[float(a) for a in alphas])
    sp = _host_ptrs(style_plans) if style_plans is not None else None
    _call("vst_cwct_factor_labels_mix", content, _ptr(content), _host_ptrs(styles), sp, al, k, float(alpha_c), _ptr(plan),
          _slots(max_slots), float(eps), n, _ptr(affines), _ptr(info))
    return affines, info


def apply_labels(x, affines, mask, plan, max_slots=0, precision="bf16x3", out=None):
    """out[:, p] = T[slot(p)] x[:, p] + t0[slot(p)], out = x where the label has no slot (vst_cwct_apply_labels); ``out`` may be ``x``."""
    n, l = _x2d("x", x)
    _f32("affines", affines, (MAX_SLOTS, n * n + n)), _u8("mask", mask, (l,)), _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    out = _out_like(out, x)
    _call("vst_cwct_apply_labels", x, _ptr(x), _ptr(out), n, l, _ptr(affines), _ptr(mask), _ptr(plan), _slots(max_slots),
          _prec(precision))
    return out


# ------------------------------------------------------------------------------------------------------- packed rows
def _code_n(sp_steps):
    if sp_steps not in (1, 2):
        raise ValueError("sp_steps must be 1 or 2")
    return 128 if sp_steps == 1 else 32


def _code(name, code, h, w):
    _f32(name, code)
    if code.numel() != h * w * 32:
        raise ValueError(f"{name} has {code.numel()} floats, a {h} x {w} image's code has {h * w * 32}")
    return code


def z_to_code(z, h, w, sp_steps, out=None):
    """z [32, H, W] (sp_steps 2) or [128, H/2, W/2] (sp_steps 1) of an H x W image -> its packed code (vst_z_to_code)."""
    import torch
    _code_n(sp_steps)
    _code("z", z, h, w)
    out = torch.empty(h * w * 32, dtype=torch.float32, device=z.device) if out is None else _code("out", out, h, w)
    _call("vst_z_to_code", z, _ptr(z), _ptr(out), 1, int(h), int(w), int(sp_steps))
    return out


def mask_to_code(mask, h, w, out=None):
    """uint8 [H, W] label map -> the label of every row of the packed code (vst_mask_to_code)."""
    import torch
    _u8("mask", mask)
    if mask.numel() != h * w:
        raise ValueError(f"mask has {mask.numel()} labels, expected {h * w}")
    out = torch.empty(h * w, dtype=torch.uint8, device=mask.device) if out is None else _u8("out", out, (h * w,))
    _call("vst_mask_to_code", mask, _ptr(mask), _ptr(out), int(h), int(w))
    return out


def stats_code(code, h, w, sp_steps, out=None):
    """{n, mean, cov} of the rows of one image's packed code (vst_cwct_stats_code)."""
    import torch
    n = _code_n(sp_steps)
    _code("code", code, h, w)
    out = torch.empty(_rec(n), dtype=torch.float64, device=code.device) if out is None else _f64("out", out, (_rec(n),))
    ws = _workspace(_lib.lib().vst_cwct_stats_code_workspace_bytes(int(h), int(w), int(sp_steps)), code)
    _call("vst_cwct_stats_code", code, _ptr(code), int(h), int(w), int(sp_steps), _ptr(out), _ptr(ws))
    return out


def stats_code_rect(code, h, w, sp_steps, rect, out=None):
    """the same over the rows whose pixels lie in rect = (y0, x0, rh, rw) (vst_cwct_stats_code_rect)."""
    import torch
    n = _code_n(sp_steps)
    _code("code", code, h, w)
    y0, x0, rh, rw = (int(v) for v in rect)
    out = torch.empty(_rec(n), dtype=torch.float64, device=code.device) if out is None else _f64("out", out, (_rec(n),))
    ws = _workspace(_lib.lib().vst_cwct_stats_code_workspace_bytes(int(h), int(w), int(sp_steps)), code)
    _call("vst_cwct_stats_code_rect", code, _ptr(code), int(h), int(w), int(sp_steps), y0, x0, rh, rw, _ptr(out), _ptr(ws))
    return out


def apply_code(code, h, w, sp_steps, affine, out=None):
    """T row + t0 on every row of one image's packed code (vst_cwct_apply_code); ``out`` may be ``code``."""
    n = _code_n(sp_steps)
    _code("code", code, h, w), _f32("affine", affine, (n * n + n,))
    out = _out_like(out, code)
    _call("vst_cwct_apply_code", code, _ptr(code), _ptr(out), int(h), int(w), int(sp_steps), _ptr(affine))
    return out


def stats_labels_code(code, h, w, mask_rows, plan, max_slots=0, out=None):
    """per-slot records of a photorealistic packed code (vst_cwct_stats_labels_code)."""
    import torch
    _code("code", code, h, w), _u8("mask_rows", mask_rows, (h * w,)), _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    out = torch.empty((MAX_SLOTS, _rec(32)), dtype=torch.float64, device=code.device) if out is None else \
        _f64("out", out, (MAX_SLOTS, _rec(32)))
    ws = _workspace(_lib.lib().vst_cwct_stats_labels_code_workspace_bytes(int(h), int(w)), code)
    _call("vst_cwct_stats_labels_code", code, _ptr(code), int(h), int(w), _ptr(mask_rows), _ptr(plan), _slots(max_slots),
          _ptr(out), _ptr(ws))
    return out


def stats_labels_code_rect(code, h, w, rect, mask_rows, plan, max_slots=0, out=None):
    """the same over a pixel rectangle (y0, x0, rh, rw) (vst_cwct_stats_labels_code_rect)."""
    import torch
    _code("code", code, h, w), _u8("mask_rows", mask_rows, (h * w,)), _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    y0, x0, rh, rw = (int(v) for v in rect)
    out = torch.empty((MAX_SLOTS, _rec(32)), dtype=torch.float64, device=code.device) if out is None else \
        _f64("out", out, (MAX_SLOTS, _rec(32)))
    ws = _workspace(_lib.lib().vst_cwct_stats_labels_code_workspace_bytes(int(h), int(w)), code)
    _call("vst_cwct_stats_labels_code_rect", code, _ptr(code), int(h), int(w), y0, x0, rh, rw, _ptr(mask_rows), _ptr(plan),
          _slots(max_slots), _ptr(out), _ptr(ws))
    return out


def apply_labels_code(code, h, w, affines, mask_rows, plan, max_slots, out=None):
    """per-slot maps on a photorealistic packed code, at most 8 slots (vst_cwct_apply_labels_code); ``out`` may be ``code``."""
    _code("code", code, h, w), _f32("affines", affines, (MAX_SLOTS, 32 * 32 + 32))
    _u8("mask_rows", mask_rows, (h * w,)), _u8("plan", plan, (_lib.LABEL_PLAN_BYTES,))
    out = _out_like(out, code)
    _call("vst_cwct_apply_labels_code", code, _ptr(code), _ptr(out), int(h), int(w), _ptr(affines), _ptr(mask_rows), _ptr(plan),
          _slots(max_slots))
    return out


# ------------------------------------------------------------------------------------------- any width and fp64 routes
# (csrc/cwct_any.hip and csrc/cwct64.hip; defined in cwct_ops_any.py with the helpers above)
from .cwct_ops_any import (apply_f64, apply_n, apply_n_f64, factor_f64, factor_n, factor_n_f64,  # noqa: E402,F401
                           prefactor_n, stats_f64, stats_n, stats_n_f64)
