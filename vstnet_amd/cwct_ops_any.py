"""The any-width and fp64 cWCT calls one by one: the ``_n`` family of csrc/cwct_any.hip (every code width N = 1..256) and the
``use_double`` route of csrc/cwct64.hip (``_f64``: N in {16, 32, 64, 128}; ``_n_f64``: any width).  Re-exported by
``vstnet_amd.cwct_ops`` (``vstnet_amd.cwct.ops.stats_n`` ...), whose conventions they keep: contiguous views at any element
offset, dtype / shape / device checks that answer without a GPU, workspaces sized by the library's ``*_workspace_bytes`` calls
(and their byte count passed where the C call takes one), ``min_tries`` and ``info`` as in ``factor``.  Records are double
[1 + N + N*N]; the fp32 affine is float32 [N*N + N], the fp64 affine double [N*N + N].  No torch implementation behind any of
these: the library refuses what it cannot run (``VstError``).
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .cwct_ops import _call, _f32, _f64, _host_ptrs, _out_like, _ptr, _rec, _u8, _workspace, _x2d

MAX_N = 256
F64_WIDTHS = (16, 32, 64, 128)


def _width(n, tuned=False):
    if tuned and n not in F64_WIDTHS:
        raise ValueError(f"N must be one of {F64_WIDTHS}, got {n}")
    if not 1 <= n <= MAX_N:
        raise ValueError(f"N must be 1..{MAX_N}, got {n}")
    return int(n)


def _stats(name, x, mask, label, out, tuned, sized):
    import torch
    n, l = _x2d("x", x)
    _width(n, tuned)
    if mask is not None:
        _u8("mask", mask, (l,))
    out = torch.empty(_rec(n), dtype=torch.float64, device=x.device) if out is None else _f64("out", out, (_rec(n),))
    ws = _workspace(getattr(_lib.lib(), name + "_workspace_bytes")(n, l), x)
    size = (ws.numel(),) if sized else ()
    _call(name, x, _ptr(x), n, l, _ptr(mask), int(label), _ptr(out), _ptr(ws), *size)
    return out


def _factor(name, content, styles, alphas, n, alpha_c, eps, min_tries, affine, tuned, sized, f64):
    import torch
    _width(n, tuned)
    _f64("content", content, (_rec(n),))
    if not 1 <= len(styles) <= _lib.MAX_STYLES or len(alphas) != len(styles):
        raise ValueError(f"factor takes 1..{_lib.MAX_STYLES} styles and as many alphas")
    for s in styles:
        _f64("style", s, (_rec(n),))
    k = len(styles)
    info = torch.zeros(2 + k, dtype=torch.int32, device=content.device)
    if min_tries is not None:
        info.copy_(torch.as_tensor(list(min_tries), dtype=torch.int32))
    if affine is None:
        affine = torch.empty(n * n + n, dtype=torch.float64 if f64 else torch.float32, device=content.device)
    else:
        (_f64 if f64 else _f32)("affine", affine, (n * n + n,))
    ws = _workspace(getattr(_lib.lib(), name + "_workspace_bytes")(n), content)
    size = (ws.numel(),) if sized else ()
    al = (C.c_float * k)(*[float(a) for a in alphas])
    _call(name, content, _ptr(content), _host_ptrs(styles), al, k, float(alpha_c), float(eps), n, _ptr(affine), _ptr(info),
          _ptr(ws), *size)
    return affine, info


def _apply(name, x, affine, out, mask, label, tuned, f64):
    n, l = _x2d("x", x)
    _width(n, tuned)
    (_f64 if f64 else _f32)("affine", affine, (n * n + n,))
    if mask is not None:
        _u8("mask", mask, (l,))
    out = _out_like(out, x)
    _call(name, x, _ptr(x), _ptr(out), n, l, _ptr(affine), _ptr(mask), int(label))
    return out


# ------------------------------------------------------------------------------------------- fp32, any width (cwct_any.hip)
def stats_n(x, mask=None, label=0, out=None):
    """{n, mean, cov} of x [N, L], N = 1..256, over all pixels or those with mask [L] == label (vst_cwct_stats_n)."""
    return _stats("vst_cwct_stats_n", x, mask, label, out, False, True)


def factor_n(content, styles, alphas, n, alpha_c=0.0, eps=2e-5, min_tries=None, affine=None):
    """(affine float32 [N*N + N], info [2 + n_styles]) at any width (vst_cwct_factor_n); ``min_tries`` as in ``factor``."""
    return _factor("vst_cwct_factor_n", content, styles, alphas, n, alpha_c, eps, min_tries, affine, False, True, False)


def prefactor_n(rec, n, eps=2e-5, out=None):
    """(prefactored record {-(n+1), mean, chol(cov)}, info [1] retries) at any width (vst_cwct_prefactor_n); ``out`` may be
    ``rec``; a record that is already prefactored comes back unchanged."""
    import torch
    _width(n)
    _f64("rec", rec, (_rec(n),))
    out = torch.empty_like(rec) if out is None else _f64("out", out, (_rec(n),))
    info = torch.zeros(1, dtype=torch.int32, device=rec.device)
    ws = _workspace(_lib.lib().vst_cwct_factor_n_workspace_bytes(n), rec)
    _call("vst_cwct_prefactor_n", rec, _ptr(rec), n, float(eps), _ptr(out), _ptr(info), _ptr(ws), ws.numel())
    return out, info


def apply_n(x, affine, out=None, mask=None, label=0):
    """out[:, p] = T x[:, p] + t0 in exact fp32 at any width (vst_cwct_apply_n); ``out`` may be ``x``."""
    return _apply("vst_cwct_apply_n", x, affine, out, mask, label, False, False)


# ------------------------------------------------------------------------------------- fp64, the tuned widths (cwct64.hip)
def stats_f64(x, mask=None, label=0, out=None):
    """two-pass fp64 {n, mean, cov} of x [N, L], N in {16, 32, 64, 128} (vst_cwct_stats_f64)."""
    return _stats("vst_cwct_stats_f64", x, mask, label, out, True, False)


def factor_f64(content, styles, alphas, n, alpha_c=0.0, eps=2e-5, min_tries=None, affine=None):
    """(affine double [N*N + N], info [2 + n_styles]) in fp64 (vst_cwct_factor_f64)."""
    return _factor("vst_cwct_factor_f64", content, styles, alphas, n, alpha_c, eps, min_tries, affine, True, False, True)


def apply_f64(x, affine, out=None, mask=None, label=0):
    """out[:, p] = float(T double(x[:, p]) + t0) with a double affine (vst_cwct_apply_f64); ``out`` may be ``x``."""
    return _apply("vst_cwct_apply_f64", x, affine, out, mask, label, True, True)


# ------------------------------------------------------------------------------------------ fp64, any width (cwct64.hip)
def stats_n_f64(x, mask=None, label=0, out=None):
    """two-pass fp64 {n, mean, cov} at any width (vst_cwct_stats_n_f64)."""
    return _stats("vst_cwct_stats_n_f64", x, mask, label, out, False, True)


def factor_n_f64(content, styles, alphas, n, alpha_c=0.0, eps=2e-5, min_tries=None, affine=None):
    """(affine double [N*N + N], info [2 + n_styles]) in fp64 at any width (vst_cwct_factor_n_f64)."""
    return _factor("vst_cwct_factor_n_f64", content, styles, alphas, n, alpha_c, eps, min_tries, affine, False, True, True)


def apply_n_f64(x, affine, out=None, mask=None, label=0):
    """out[:, p] = float(T double(x[:, p]) + t0) at any width, fp64 accumulation (vst_cwct_apply_n_f64); ``out`` may be ``x``."""
    return _apply("vst_cwct_apply_n_f64", x, affine, out, mask, label, False, True)
