"""cWCT — drop-in for the reference's ``models.cWCT.cWCT`` on MI355X.

Same constructor and methods as models/cWCT.py:9-262 (``transfer``, ``interpolation`` and the
public-by-convention helpers).  Differences, all documented in DESIGN.md:
  * ``transfer`` without masks implements the intended per-sample semantics (the fork's batched
    ``whitening`` raises on [B,N,L] input);
  * the Cholesky-failure path retries with the reference's jitter schedule but never enters pdb;
  * masks must have the feature resolution (the fork does not resize them, cWCT.py:72-73): a
    mismatch raises ValueError instead of indexing out of range;
  * ``use_double=True`` (cWCT.py:13-16,35-47,66,106,220,238,259; no script of the reference sets it, and in this fork the flag
    traps into pdb, :36) runs true fp64 two-pass statistics, an fp64 Cholesky / inverse / mix and an fp64-accumulating apply
    (csrc/cwct64.hip) on the dense NCHW code: a fidelity option — packed codes are materialised first, masked transfers go
    label by label like the reference's loop.  Without it the mean / covariance combine is fp64, the rest fp32;
  * a batch is factored like the reference's [B,N,N] stack: a sample that needs Cholesky jitter jitters every sample
    (cWCT.py:122-128); ``transfer_with_stats`` / ``transfer_with_plan`` (this repo's cached-style extensions) are per sample;
  * codes of any other width N = 1..256 (a RevResNet with another hidden_dim) run on the width-generic kernels
    (csrc/cwct_any.hip, ``WIDTH_ROUTES``): the apply there is exact fp32 whatever ``precision`` says, masked transfers go label
    by label, and the single-pass masked extension (``plan_masks`` / ``transfer_with_plan``) is not available;
  * ``interpolation`` takes label maps (``cmask``, ``smask_list``): the reference's scripts say "mask is not supported" there
    (video_transfer.py:198-201, image_transfer.py:192-196).  Per label it is the reference's ``interpolation`` on the gathered
    columns, for the labels valid against every style map (``INTERP_ROUTES``); the cached forms take lists of styles.  The
    masked ``transfer`` is the one-style case of the same code (weight 1, ``alpha_c`` = 0): one plan form (``MaskPlan``, lists
    per style), one plan builder (vst_label_hist per map + vst_label_plan_hists), one factor call (vst_cwct_factor_labels_mix).
  * every transfer call takes ``strength=`` (a map in [0, 1] at the code's resolution, or a ``bind_strength`` object): the
    result is x + s (A(x) - x) per code pixel, the map form of ``alpha_c`` ("Strength maps").
  * ``frame_strength`` makes ONE frame's strength map on the device, on the current stream, from the frame's 8-bit matte and / or
    its label map and a ``strength_table``: what a video loop calls per frame where ``bind_strength`` (host map, upload,
    synchronisation) is right once per clip.
  * ``interpolation`` and ``transfer_with_stats`` take ``style_map=`` (K weight planes at the code's resolution, or a
    ``bind_style_map`` object) in place of the K weights: the result is sum_k w_k(p) A_k(x) per code pixel, the map form of
    ``alpha_s`` ("Style maps").  Not on the masked routes.
  * ``frame_style_map`` makes ONE frame's style map on the device, on the current stream, from the frame's 8-bit weight planes:
    what a video loop calls per frame where ``bind_style_map`` (host planes, validation, upload, synchronisation) is right once
    per clip.
All device work goes through libvstnet_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .code import PackedCode

_SUPPORTED_N = (16, 32, 64, 128)          # widths with tuned kernels (csrc/cwct.hip, cwct64.hip)
_MAX_N = 256                               # any other 1 <= N <= _MAX_N: the width-generic kernels (csrc/cwct_any.hip)


def _stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _call(device, name, *args):
    """One call of the library on `device`'s current stream (appended as the last argument); a non-zero status raises."""
    with torch.cuda.device(device):
        _lib.check(getattr(_lib.lib(), name)(*args, _stream_ptr()), name)


class MaskPlan:
    """What the masked transfer derives from the label maps alone (cWCT.plan_masks, cWCT.plan_frame): per sample the uint8
    maps and the label -> slot table, all on the device; optionally the per-slot style statistics (cWCT.bind_style).  The style
    side is a list per style whoever built the plan: one style is a list of one."""

    def __init__(self, content_shape, style_shapes):
        self.content_shape = tuple(content_shape)
        self.style_shapes = [tuple(sh) for sh in style_shapes]      # every style code's shape
        self.cm, self.tables, self.max_slots = [], [], 0            # 0 = unknown (launches cover all 32 slots)
        self.cm_rows = None        # the content label maps in a PackedCode's row order (made on first use)
        self.sms = [[] for _ in self.style_shapes]      # sms[i][b] = style i's label map
        self.styles = None         # bind_style: styles[i][b] = prefactored per-slot records of style i
        self.bindings = None       # plan_frame: every style's StyleBinding, the style side keyed by LABEL; tables[b] then maps RAW labels
        self.flags = None          # device int32 [1]: VST_MASK_* bits of a per-frame plan (read when the frame retires)
        self.work = None           # a per-frame plan's buffers for statistics / affines / info (the frame's ring slot)


class StyleBinding:
    """The style side of a masked transfer keyed by label (cWCT.bind_style_labels): the style map's histogram, a plan of the
    style map against itself (every label with more than 10 style pixels has a slot) and the per-slot statistics of the style
    code.  It does not depend on any content map, so a clip whose masks change per frame reads the style code once."""

    def __init__(self, shape, hist, plan, stats):
        self.shape, self.hist, self.plan, self.stats = tuple(shape), hist, plan, stats


class StrengthMap:
    """A strength map bound to a code shape (cWCT.bind_strength): `dense` = float32 [B, cH * cW] on the device, one strength
    per code pixel in image order (what the dense routes blend with, vst_cwct_blend); `rows` = float32 [B, rows] in a
    PackedCode's row order (vst_map_to_code; what the packed apply kernels blend with), or None where the shape has no packed
    form.  Complete when bind_strength returns, read-only afterwards: frames in flight on several streams share it."""

    def __init__(self, code_shape, dense, rows):
        self.code_shape, self.dense, self.rows = tuple(code_shape), dense, rows


class StyleMap:
    """A style map bound to a code shape (cWCT.bind_style_map): `dense` = float32 [B, K, cH * cW] on the device, the weight of
    every style per code pixel in image order (what the dense routes accumulate with, vst_cwct_mix_acc); `rows` = float32
    [B, K, rows], the K planes in a PackedCode's row order (vst_map_to_code; what the packed mix kernels read), or None where
    the shape has no packed form.  Complete when bind_style_map returns, read-only afterwards: frames in flight share it."""

    def __init__(self, code_shape, dense, rows):
        self.code_shape, self.dense, self.rows = tuple(code_shape), dense, rows
        self.K = int(dense.shape[1])


class cWCT(nn.Module):
    """Cholesky decomposition based WCT (HIP implementation)."""

    def __init__(self, eps=2e-5, use_double=False, resize_masks=False, precision=None):
        super().__init__()
        # arithmetic of the apply (y = T x + t0): "fp32" = exact fp32 kernels for every N; anything else lets unmasked
        # N >= 64 codes (artistic mode) run on bf16 MFMA with split operands.  Follows RevResNet's knob by default.
        precision = precision or _lib.default_precision()
        if precision == "auto":               # (RevResNet's self-calibrating mode: nothing to decide here)
            precision = "bf16x3"
        if precision not in ("fp32", "bf16x3", "f16x2", "f16x2h"):
            raise ValueError("precision must be one of ['auto', 'bf16x3', 'f16x2', 'f16x2h', 'fp32']")
        self.precision = precision
        self.eps = eps
        self.use_double = bool(use_double)
        # upstream CAP-VSTNet resized the label maps to the feature resolution (NEAREST, cWCT.py:191-197); this
        # fork uses them as they are (:72-73), which only fits photorealistic codes.  Opt in to restore it.
        self.resize_masks = resize_masks
        self._ws = None
        self.last_info = None      # device int32 [2+n_styles]: content retries, overflow flag, style retries
        self.last_route = None     # key of ROUTES the last transfer took
        self.last_strength = None  # how the last transfer took its strength map: "packed_rows", "dense" or None (no map)
        self.last_style_map = None # how the last transfer took its style map: "packed_rows", "dense" or None (no map)

    # ------------------------------------------------------------------ low-level wrappers
    def _workspace(self, nbytes, device):
        """Statistics workspace, one per (device, stream)."""
        if self._ws is None:
            self._ws = {}
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            self._ws[key] = ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        return ws

    @staticmethod
    def _prep(x):
        if not x.is_cuda:
            raise RuntimeError("vstnet_amd.cWCT runs on ROCm devices only (no CPU fallback)")
        return x.detach().to(torch.float32).contiguous()

    def stats(self, x2d, mask=None, label=0, out=None):
        """mean / covariance of a [N,L] feature matrix (optionally of the pixels with mask==label)
        -> device double tensor [1+N+N*N] = {n, mean, cov}  (cWCT.py:138-144 / 153-157).  out: where to write it."""
        N, Lp = x2d.shape
        fam = self._family(N)
        fn = "vst_cwct_stats" + fam
        if out is None:
            out = torch.empty(1 + N + N * N, dtype=torch.float64, device=x2d.device)
        ws = self._workspace(getattr(_lib.lib(), fn + "_workspace_bytes")(N, Lp), x2d.device)
        sized = (ws.numel(),) if "_n" in fam else ()       # the width-generic calls check the size of their workspace
        _call(x2d.device, fn, _ptr(x2d), N, Lp, _ptr(mask), int(label), _ptr(out), _ptr(ws), *sized)
        return out

    def _family(self, N):
        """Suffix of the kernel family that serves an N-channel code: "" / "_f64" at the tuned widths (csrc/cwct.hip,
        cwct64.hip), "_n" / "_n_f64" at any other (csrc/cwct_any.hip)."""
        if N in _SUPPORTED_N:
            return "_f64" if self.use_double else ""
        self._check_width(N)
        return "_n_f64" if self.use_double else "_n"

    def stats_code(self, z, b, out=None):
        """stats() of image b of a PackedCode (all pixels), on the packed rows (vst_cwct_stats_code)."""
        rows = z.applied()[b]
        H, W = z.image_hw
        N = z.shape[1]
        if out is None:
            out = torch.empty(1 + N + N * N, dtype=torch.float64, device=rows.device)
        ws = self._workspace(_lib.lib().vst_cwct_stats_code_workspace_bytes(H, W, z.sp_steps), rows.device)
        _call(rows.device, "vst_cwct_stats_code", _ptr(rows), H, W, z.sp_steps, _ptr(out), _ptr(ws))
        return out

    # ------------------------------------------------------------------ the ONE place where a transfer's route is chosen
    # (code layout x mask x N x slot count x use_double) -> which kernels run.  The arithmetic of the dense applies (exact fp32
    # vs bf16 split operands for N >= 64) is the `precision` argument of vst_cwct_apply_prec / vst_cwct_apply_labels and is
    # chosen inside the library; everything else is decided here and recorded in `last_route`.
    ROUTES = {
        "packed_rows": "unmasked, code in the coupling blocks' layout: vst_cwct_stats_code + factor; the map stays pending and "
                       "is applied by the inverse pass (vst_revnet_decode)",
        "dense": "unmasked NCHW code: vst_cwct_stats + factor + vst_cwct_apply_prec",
        "masked_packed_rows": "masked, photorealistic packed code, 1..8 label slots known: vst_cwct_stats_labels_code + "
                              "vst_cwct_factor_labels_mix (one style, weight 1); per-row maps pending (vst_revnet_decode_labels)",
        "masked_single_pass": "masked NCHW code, N in {32, 64, 128}: vst_label_hist x 2 + vst_label_plan_hists, vst_cwct_stats_labels "
                              "(content, style) + vst_cwct_factor_labels_mix (one style, weight 1) + vst_cwct_apply_labels",
        "masked_per_label": "masked NCHW code, N = 16: one vst_cwct_stats / factor / apply per valid label",
        "dense_f64": "use_double, unmasked: vst_cwct_stats_f64 + factor_f64 + apply_f64 on the NCHW code",
        "masked_per_label_f64": "use_double, masked: the fp64 calls per valid label (the reference's loop, cWCT.py:83-103)",
    }

    # Codes of any other width (1 <= N <= 256: RevResNet(hidden_dim=...) gives N = 2 * hidden_dim) take one of these instead.
    # Their apply is exact fp32 whatever `precision` says (like the generic RevResNet path); no packed or single-pass forms.
    WIDTH_ROUTES = {
        "any_width_dense": "unmasked NCHW code, N outside {16, 32, 64, 128}: vst_cwct_stats_n + factor_n + apply_n (exact fp32)",
        "any_width_masked_per_label": "masked NCHW code, N outside {16, 32, 64, 128}: one vst_cwct_stats_n / factor_n / apply_n "
                                      "per valid label (exact fp32)",
        "any_width_dense_f64": "use_double, unmasked, N outside {16, 32, 64, 128}: vst_cwct_stats_n_f64 + factor_n_f64 + "
                               "apply_n_f64",
        "any_width_masked_per_label_f64": "use_double, masked, N outside {16, 32, 64, 128}: the fp64 _n calls per valid label",
    }

    # interpolation(..., cmask, smask_list): several styles and alpha_c per label.  The calls are those of the masked transfer
    # with K styles instead of one (a label is valid against EVERY style map); the masked transfer is the K = 1, weight 1,
    # alpha_c = 0 case of the same code and keeps its own route names.
    INTERP_ROUTES = {
        "interp_masked_single_pass": "masked NCHW code, N in {32, 64, 128}: vst_label_hist x (1 + K) + vst_label_plan_hists, "
                                     "vst_cwct_stats_labels (content and every style) + vst_cwct_factor_labels_mix + "
                                     "vst_cwct_apply_labels",
        "interp_masked_packed_rows": "masked, photorealistic packed code, 1..8 label slots: vst_cwct_stats_labels_code + "
                                     "vst_cwct_factor_labels_mix; per-row maps pending (vst_revnet_decode_labels)",
        "interp_masked_per_label": "N = 16, any other width, or use_double: one statistics call per style, one factor (all styles, "
                                   "alpha_c) and one apply per label valid against every style map",
    }

    @staticmethod
    def interp_route(packed, N, sp_steps=2, max_slots=0, use_double=False):
        """Name of the route (a key of INTERP_ROUTES) of a masked interpolation; arguments as for route()."""
        cWCT._check_width(N)
        if use_double or N not in (32, 64, 128):
            return "interp_masked_per_label"
        return "interp_" + cWCT.route(packed, True, N, sp_steps, max_slots)

    @staticmethod
    def check_mix(n_styles, alpha_s_list, n_masks=None):
        """The argument rules of a style mix: as many weights as styles (AssertionError, like the reference's assert), at most
        MAX_STYLES styles and one label map per style (ValueError)."""
        assert n_styles == len(alpha_s_list), "one weight per style (models/cWCT.py:207)"
        if not 1 <= n_styles <= _lib.MAX_STYLES:
            raise ValueError(f"a mix takes at least 1 and at most {_lib.MAX_STYLES} styles, got {n_styles}")
        if n_masks is not None and n_masks != n_styles:
            raise ValueError(f"one style label map per style: {n_masks} maps for {n_styles} styles")

    @staticmethod
    def width_route(masked, use_double=False):
        """Name of the route (a key of WIDTH_ROUTES) for a code whose width has no tuned kernels."""
        r = "any_width_masked_per_label" if masked else "any_width_dense"
        return r + "_f64" if use_double else r

    @staticmethod
    def _check_width(N):
        if not 1 <= N <= _MAX_N:
            raise NotImplementedError(f"HIP cWCT supports 1 <= N <= {_MAX_N}, got {N}")

    @staticmethod
    def route(packed, masked, N, sp_steps=2, max_slots=0, use_double=False):
        """Name of the route (a key of ROUTES) for a code that is / is not a usable PackedCode (`packed`: no pending map, not
        written to), with / without masks, N channels, `max_slots` label slots known to the host (0 = never read back)."""
        if N not in _SUPPORTED_N:
            raise NotImplementedError(f"HIP cWCT supports N in {_SUPPORTED_N}, got {N}")
        if use_double:
            return "masked_per_label_f64" if masked else "dense_f64"
        if not masked:
            return "packed_rows" if packed and ((N == 32 and sp_steps == 2) or (N == 128 and sp_steps == 1)) else "dense"
        if N == 16:
            return "masked_per_label"
        if packed and N == 32 and sp_steps == 2 and 1 <= int(max_slots) <= 8:
            return "masked_packed_rows"
        return "masked_single_pass"

    def _route_of(self, content_feat, masked, max_slots=0, mix=False):
        """The route of this call, recorded in `last_route`.  mix: a masked call that names its styles' weights or alpha_c (the
        interpolation); it runs the code of the masked transfer and differs in the name only (INTERP_ROUTES)."""
        N = content_feat.shape[1]
        layout = (self._is_packed_code(content_feat), N, getattr(content_feat, "sp_steps", 2), max_slots, self.use_double)
        if mix:
            r = self.interp_route(*layout)
        elif N not in _SUPPORTED_N:
            self._check_width(N)
            r = self.width_route(masked, self.use_double)
        else:
            r = self.route(layout[0], masked, *layout[1:])
        self.last_route = r
        return r

    @staticmethod
    def _is_packed_code(x):
        """A code still in the coupling blocks' layout, no cWCT pending on it (code.py); use_double works on dense codes."""
        return isinstance(x, PackedCode) and not x.pending and not x.stale

    def factor(self, content_stats, style_stats_list, alphas, alpha_c, N, min_tries=None):
        """{T, t0} with T = (sum_i a_i chol(Cs_i) [blended with chol(Cc)]) * chol(Cc)^-1.  min_tries: device int32
        [2+n_styles] jitter retries to start from (the batch coupling of `interpolation`)."""
        n = len(style_stats_list)
        dev = content_stats.device
        fam = self._family(N)
        fn = "vst_cwct_factor" + fam
        info = torch.zeros(2 + n, dtype=torch.int32, device=dev) if min_tries is None else min_tries.clone()
        ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in style_stats_list])
        al = (C.c_float * n)(*[float(a) for a in alphas])
        # use_double: fp64 Cholesky / inverse / mix and a DOUBLE affine record
        affine = torch.empty(N * N + N, dtype=torch.float64 if self.use_double else torch.float32, device=dev)
        work = ()
        if fam:                                  # every family but the tuned fp32 one keeps its matrices in a workspace
            fws = torch.empty(getattr(_lib.lib(), fn + "_workspace_bytes")(N), dtype=torch.uint8, device=dev)
            work = (_ptr(fws), fws.numel()) if "_n" in fam else (_ptr(fws),)
        _call(dev, fn, _ptr(content_stats), ptrs, al, n, float(alpha_c), float(self.eps), N, _ptr(affine), _ptr(info), *work)
        self.last_info = info
        return affine

    def apply(self, x2d, affine, out=None, mask=None, label=0):
        N, Lp = x2d.shape
        if out is None:
            out = torch.empty_like(x2d)
        fam = self._family(N)
        # the tuned fp32 family takes `precision`; the others are exact fp32 (or fp64-accumulating) whatever it says
        fn, prec = ("vst_cwct_apply" + fam, ()) if fam else ("vst_cwct_apply_prec", (_lib.PRECISIONS[self.precision],))
        _call(x2d.device, fn, _ptr(x2d), _ptr(out), N, Lp, _ptr(affine), _ptr(mask), int(label), *prec)
        return out

    @staticmethod
    def _identity_stats(N, device):
        s = torch.zeros(1 + N + N * N, dtype=torch.float64, device=device)
        s[0] = 2.0
        s[1 + N:] = torch.eye(N, dtype=torch.float64, device=device).reshape(-1)
        return s

    # ------------------------------------------------------------------ strength maps
    # alpha_c is linear in the affine map: ((1-a) Ls + a Lc) Lc^-1 (x - mc) + (1-a) ms + a mc = (1-a) A(x) + a x.  A strength
    # s(p) per code pixel is that parameter as a map: y = x + s (A(x) - x).  It composes with everything that produces A.
    def bind_strength(self, strength, code_shape, device):
        """A float map at the code's resolution -> StrengthMap.  strength: [cH, cW] (shared by the B samples) or [B, 1, cH, cW],
        a tensor or numpy, values in [0, 1] (1 = the full transfer, 0 = the content code); code_shape = the content code's
        [B, N, cH, cW].  The object is complete before this returns (one synchronisation) and is then only read."""
        B, N, cH, cW = (int(v) for v in code_shape)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("vstnet_amd.cWCT runs on ROCm devices only (no CPU fallback)")
        m = strength if torch.is_tensor(strength) else torch.from_numpy(np.ascontiguousarray(np.asarray(strength, dtype=np.float32)))
        m = m.detach().to(torch.float32)
        if m.dim() == 2 and tuple(m.shape) == (cH, cW):
            m = m.reshape(1, cH * cW).expand(B, cH * cW)
        elif m.dim() == 4 and tuple(m.shape) == (B, 1, cH, cW):
            m = m.reshape(B, cH * cW)
        else:
            raise ValueError(f"a strength map has the code's resolution: [{cH}, {cW}] or [{B}, 1, {cH}, {cW}], got {tuple(m.shape)}")
        lo, hi = float(m.min()), float(m.max())
        if not (lo >= 0.0 and hi <= 1.0):                # (also rejects NaN)
            raise ValueError(f"strength values must lie in [0, 1], got [{lo}, {hi}]")
        dense = m.to(device).contiguous()
        rows = None
        sp = {32: 2, 128: 1}.get(N)
        H, W = (cH, cW) if sp == 2 else (2 * cH, 2 * cW)
        if sp is not None and H % 4 == 0 and W % 4 == 0:
            rows = torch.empty_like(dense)
            with torch.cuda.device(device):
                for b in range(B):
                    _call(device, "vst_map_to_code", _ptr(dense[b]), _ptr(rows[b]), H, W, sp)
        with torch.cuda.device(device):
            torch.cuda.current_stream(device).synchronize()
        return StrengthMap((B, N, cH, cW), dense, rows)

    # ---- one map per frame, made on the device (vst_strength_frame): a matte and / or a strength per label of the frame's map
    @staticmethod
    def strength_table(spec, default=1.0, device=None):
        """The 256-entry table of per-label strengths: spec = {label: strength} or a string "12:0.2,20:0"; every other label
        gets `default`.  float32 [256], on `device` when given.  A label outside 0..255 or a value outside [0, 1]: ValueError."""
        if isinstance(spec, str):
            pairs = []
            for item in (s.strip() for s in spec.split(",")):
                if not item:
                    continue
                try:
                    k, v = item.split(":")
                    pairs.append((int(k.strip()), float(v.strip())))
                except ValueError:
                    raise ValueError(f"a strength table reads LABEL:STRENGTH[,LABEL:STRENGTH...], got {item!r}") from None
        else:
            pairs = [(k, v) for k, v in dict(spec).items()]
        if not 0.0 <= float(default) <= 1.0:
            raise ValueError(f"the default strength must lie in [0, 1], got {default}")
        t = np.full(256, float(default), np.float32)
        for k, v in pairs:
            if int(k) != k or not 0 <= int(k) <= 255:
                raise ValueError(f"a label is an integer in 0..255, got {k}")
            if not 0.0 <= float(v) <= 1.0:               # (also rejects NaN)
                raise ValueError(f"strength values must lie in [0, 1], got {v} for label {k}")
            t[int(k)] = float(v)
        t = torch.from_numpy(t)
        return t if device is None else t.to(device)

    @staticmethod
    def _frame_geometry(code_shape):
        B, N, cH, cW = (int(v) for v in code_shape)
        sp = {32: 2, 128: 1}.get(N)
        H, W = (cH, cW) if sp == 2 else (2 * cH, 2 * cW)
        if B != 1 or sp is None or H % 4 or W % 4 or H < 8 or W < 8:
            raise ValueError(f"a frame's strength map belongs to one packed code: [1, 32, H, W] or [1, 128, H/2, W/2] with H, W "
                             f"multiples of 4, got {tuple(code_shape)}")
        return (B, N, cH, cW), sp, H, W

    @staticmethod
    def empty_strength(code_shape, device):
        """The buffers of one frame's StrengthMap (frame_strength's `out`): a ring slot makes them once."""
        shape, _, _, _ = cWCT._frame_geometry(code_shape)
        n = shape[2] * shape[3]
        return StrengthMap(shape, torch.empty((1, n), dtype=torch.float32, device=device),
                           torch.empty((1, n), dtype=torch.float32, device=device))

    @staticmethod
    def frame_strength(code_shape, matte=None, labels=None, table=None, out=None):
        """One frame's StrengthMap on the current stream (vst_strength_frame): matte = uint8 [H,W] grey and / or labels = uint8
        [H,W], both device tensors at the stylised frame size, table = float32 [256] on the device (strength_table; needed with
        labels).  s = v / 255 (after Pillow's BOX for artistic codes), table[label], or their product.  With `out` (empty_strength)
        nothing is allocated; nothing synchronises: the map is complete in stream order, for a transfer queued behind it."""
        shape, sp, H, W = cWCT._frame_geometry(code_shape)
        if matte is None and labels is None:
            raise ValueError("frame_strength needs a matte, a label map or both")
        dev = (matte if matte is not None else labels).device
        for name, t in (("matte", matte), ("labels", labels)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != (H, W) or not t.is_cuda
                                  or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"{name} must be a contiguous uint8 [{H}, {W}] tensor on the GPU, got "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if labels is not None and (table is None or not torch.is_tensor(table) or table.dtype != torch.float32
                                   or tuple(table.shape) != (256,) or table.device != dev or not table.is_contiguous()):
            raise ValueError(f"labels need a float32 [256] strength table on {dev} (cWCT.strength_table)")
        if out is None:
            out = cWCT.empty_strength(shape, dev)
        elif not isinstance(out, StrengthMap) or out.code_shape != shape or out.rows is None or out.dense.device != dev \
                or any(t.dtype != torch.float32 or tuple(t.shape) != (1, shape[2] * shape[3]) or not t.is_contiguous()
                       for t in (out.dense, out.rows)):
            raise ValueError(f"out must be a StrengthMap of shape {shape} on {dev} with dense and rows buffers")
        _call(dev, "vst_strength_frame", _ptr(matte), _ptr(labels), _ptr(table if labels is not None else None), _ptr(out.dense),
              _ptr(out.rows), H, W, sp)
        return out

    def _strength_of(self, strength, content_feat):
        """The StrengthMap of this call (None without a map): a bound one must fit the code, a raw map is bound now."""
        self.last_strength = None
        if strength is None:
            return None
        shape = tuple(int(v) for v in content_feat.shape)
        if isinstance(strength, StrengthMap):
            if strength.code_shape != shape or strength.dense.device != content_feat.device:
                raise ValueError(f"the strength map was bound for a code of shape {strength.code_shape} on "
                                 f"{strength.dense.device}, got {shape} on {content_feat.device}")
            return strength
        return self.bind_strength(strength, shape, content_feat.device)

    def _strength_rows(self, sm):
        """The rows a PackedCode result carries (None without a map)."""
        if sm is None:
            return None
        if sm.rows is None:
            raise ValueError("this strength map has no packed rows (its code shape has no packed form)")
        self.last_strength = "packed_rows"
        return sm.rows

    def _blend(self, x2d, y2d, sm, b, out):
        """out = x + s (y - x) per pixel of an [N, L] code and its cWCT (vst_cwct_blend; out may be x2d or y2d)."""
        N, Lp = x2d.shape
        _call(x2d.device, "vst_cwct_blend", _ptr(x2d), _ptr(y2d), _ptr(sm.dense[b]), _ptr(out), N, Lp)
        self.last_strength = "dense"

    # ------------------------------------------------------------------ style maps
    # `interpolation` whitens once and mixes the colourings linearly: for weights that sum to 1 it is sum_k a_k A_k(c) with A_k
    # the affine map of style k alone at the same alpha_c.  Weights w_k(p) per code pixel are alpha_s as a map; what changes is
    # the apply: K maps per image, a weight per row and map.
    STYLE_MAP_SUM_TOL = 1e-5

    def bind_style_map(self, weights, code_shape, device):
        """K weight planes at the code's resolution -> StyleMap.  weights: float [B or 1, K, cH, cW] or [K, cH, cW], a tensor or
        numpy, K = 2..8; finite, >= 0 and summing to 1 within 1e-5 at every pixel (ValueError otherwise); code_shape = the
        content code's [B, N, cH, cW].  Complete before this returns (one synchronisation), only read afterwards."""
        B, N, cH, cW = (int(v) for v in code_shape)
        m = weights if torch.is_tensor(weights) else torch.from_numpy(np.ascontiguousarray(np.asarray(weights, dtype=np.float32)))
        m = m.detach().to(torch.float32).cpu()
        if m.dim() == 3:
            m = m.unsqueeze(0)
        if m.dim() != 4 or m.shape[0] not in (1, B) or tuple(m.shape[2:]) != (cH, cW):
            raise ValueError(f"a style map has the code's resolution: [K, {cH}, {cW}] or [{B} or 1, K, {cH}, {cW}], got "
                             f"{tuple(m.shape)}")
        K = int(m.shape[1])
        if not 2 <= K <= _lib.MAX_STYLES:
            raise ValueError(f"a style map mixes 2..{_lib.MAX_STYLES} styles, got {K} planes")
        if not bool(torch.isfinite(m).all()):
            raise ValueError("style map weights must be finite")
        if float(m.min()) < 0.0:
            raise ValueError(f"style map weights must be >= 0, got {float(m.min())}")
        dev_sum = float((m.sum(dim=1) - 1.0).abs().max())
        if not dev_sum <= self.STYLE_MAP_SUM_TOL:
            raise ValueError(f"style map weights must sum to 1 at every pixel (within {self.STYLE_MAP_SUM_TOL}), off by {dev_sum}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("vstnet_amd.cWCT runs on ROCm devices only (no CPU fallback)")
        dense = m.reshape(m.shape[0], K, cH * cW).expand(B, K, cH * cW).contiguous().to(device)
        rows = None
        sp = {32: 2, 128: 1}.get(N)
        H, W = (cH, cW) if sp == 2 else (2 * cH, 2 * cW)
        if sp is not None and H % 4 == 0 and W % 4 == 0:
            rows = torch.empty_like(dense)
            for b in range(B):
                for k in range(K):
                    _call(device, "vst_map_to_code", _ptr(dense[b, k]), _ptr(rows[b, k]), H, W, sp)
        with torch.cuda.device(device):
            torch.cuda.current_stream(device).synchronize()
        return StyleMap((B, N, cH, cW), dense, rows)

    # ---- one map per frame, made on the device (vst_style_frame): the frame's 8-bit weight planes
    @staticmethod
    def empty_style_map(code_shape, K, device):
        """The buffers of one frame's StyleMap of K styles (frame_style_map's `out`): a ring slot makes them once."""
        shape, _, _, _ = cWCT._frame_geometry(code_shape)
        K = int(K)
        if not 2 <= K <= _lib.MAX_STYLES:
            raise ValueError(f"a style map mixes 2..{_lib.MAX_STYLES} styles, got {K}")
        n = shape[2] * shape[3]
        return StyleMap(shape, torch.empty((1, K, n), dtype=torch.float32, device=device),
                        torch.empty((1, K, n), dtype=torch.float32, device=device))

    @staticmethod
    def frame_style_map(code_shape, planes, out=None, flags=None):
        """One frame's StyleMap on the current stream (vst_style_frame): planes = uint8 [P,H,W] grey, a contiguous device tensor
        at the stylised frame size; P = 1: the weight of the second of two styles (K = 2), P = 2..8: one plane per style (K = P),
        w_k = v_k / sum_j v_j (after Pillow's BOX for artistic codes): the maps bind_style_map makes of
        utils.style_map_weights' planes.  flags: an int32 [1] device tensor the caller has cleared; bit 0 is set when every
        plane is 0 at some pixel, which then takes the first style alone.  With `out` (empty_style_map) nothing is allocated;
        nothing synchronises: the map is complete in stream order, for a transfer queued behind it."""
        shape, sp, H, W = cWCT._frame_geometry(code_shape)
        if not torch.is_tensor(planes) or planes.dtype != torch.uint8 or planes.dim() != 3 or not planes.is_cuda \
                or not 1 <= planes.shape[0] <= _lib.MAX_STYLES or tuple(planes.shape[1:]) != (H, W) or not planes.is_contiguous():
            raise ValueError(f"planes must be a contiguous uint8 [P, {H}, {W}] tensor on the GPU with P = 1..{_lib.MAX_STYLES}, "
                             f"got {getattr(planes, 'dtype', type(planes))} {tuple(getattr(planes, 'shape', ()))}")
        dev, P = planes.device, int(planes.shape[0])
        K = 2 if P == 1 else P
        if flags is not None and (not torch.is_tensor(flags) or flags.dtype != torch.int32 or flags.numel() != 1
                                  or flags.device != dev):
            raise ValueError(f"flags must be an int32 [1] tensor on {dev}")
        if out is None:
            out = cWCT.empty_style_map(shape, K, dev)
        elif not isinstance(out, StyleMap) or out.code_shape != shape or out.rows is None or out.dense.device != dev \
                or any(t.dtype != torch.float32 or tuple(t.shape) != (1, K, shape[2] * shape[3]) or not t.is_contiguous()
                       for t in (out.dense, out.rows)):
            raise ValueError(f"out must be a StyleMap of {K} styles and shape {shape} on {dev} with dense and rows buffers")
        _call(dev, "vst_style_frame", _ptr(planes), P, _ptr(out.dense), _ptr(out.rows), _ptr(flags), H, W, sp)
        return out

    def _style_map_of(self, style_map, content_feat, n_styles):
        """The StyleMap of this call: a bound one must fit the code and the number of styles, a raw one is bound now."""
        shape = tuple(int(v) for v in content_feat.shape)
        if isinstance(style_map, StyleMap):
            if style_map.code_shape != shape or style_map.dense.device != content_feat.device:
                raise ValueError(f"the style map was bound for a code of shape {style_map.code_shape} on "
                                 f"{style_map.dense.device}, got {shape} on {content_feat.device}")
            smap = style_map
        else:
            smap = self.bind_style_map(style_map, shape, content_feat.device)
        if smap.K != n_styles:
            raise ValueError(f"the style map has {smap.K} planes for {n_styles} styles")
        return smap

    def _mix_acc(self, a2d, w, out2d, first):
        """out = first ? w a : out + w a per pixel of an [N, L] code (vst_cwct_mix_acc)."""
        N, Lp = a2d.shape
        _call(a2d.device, "vst_cwct_mix_acc", _ptr(a2d), _ptr(w), _ptr(out2d), N, Lp, int(bool(first)))

    def _transfer_style_map(self, content_feat, styles_of, K, alpha_c, smap, sm, couple, content_stats=None):
        """sum_k w_k A_k(x) [then the strength blend]: styles_of(b) = the K style statistics of sample b; K factor calls per
        sample, each factor(cs, [style_k], [1.0], alpha_c).  couple: the batch's jitter coupling of `interpolation`, over all K."""
        B, N, cH, cW = content_feat.shape
        packed = self._route_of(content_feat, masked=False) == "packed_rows"
        if packed and N == 128 and K > 2:        # two sets of fragments fill the LDS: more styles go through the dense code
            packed, self.last_route = False, "dense_f64" if self.use_double else "dense"
        in_dtype = content_feat.dtype
        c = None if packed else self._prep(content_feat).reshape(B, N, -1)
        if content_stats is None:
            stats = [(self.stats_code(content_feat, b) if packed else self.stats(c[b]), styles_of(b)) for b in range(B)]
        else:
            stats = [(self._content_record(content_stats, content_feat, None, b), styles_of(b)) for b in range(B)]
        affines, infos = [], []
        for cs, ss in stats:
            per = []
            for st in ss:
                per.append(self.factor(cs, [st], [1.0], alpha_c, N))
                infos.append(self.last_info)
            affines.append(per)
        if couple and B > 1:
            need = torch.stack(infos).max(dim=0).values
            need[1] = 0
            affines = [[self.factor(cs, [st], [1.0], alpha_c, N, min_tries=need) for st in ss] for cs, ss in stats]
        if packed:
            if smap.rows is None:
                raise ValueError("this style map has no packed rows (its code shape has no packed form)")
            self.last_style_map = "packed_rows"
            return content_feat.with_affines(torch.stack([torch.stack(per) for per in affines]), self._strength_rows(sm),
                                             mix=smap.rows)
        out = torch.empty_like(c)
        tmp = torch.empty_like(c[0])             # the K plain applies land here one after the other: memory does not grow with K
        for b in range(B):
            for k in range(K):
                self.apply(c[b], affines[b][k], out=tmp)
                self._mix_acc(tmp, smap.dense[b, k], out[b], k == 0)
            if sm is not None:
                self._blend(c[b], out[b], sm, b, out[b])
        self.last_style_map = "dense"
        return out.to(in_dtype).reshape(B, N, cH, cW)

    # ------------------------------------------------------------------ statistics window
    # The affine map is global to a frame, so a change of the frame's statistics recolours every pixel of it.  A video loop can
    # steady the map by whitening a frame with the statistics of the frame AND of the frames before it: records of pixel sets
    # combine in closed form (vst_cwct_stats_pool), between the statistics and the factor calls that exist.
    def _check_record_out(self, out, shape, device):
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device=device)
        if not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != tuple(shape) or out.device != device \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float64 {tuple(shape)} tensor on {device}, got "
                             f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
        return out

    def frame_stats(self, content_feat, plan=None, b=0, out=None, by_label=False):
        """The content record(s) the route of this code computes for sample b, and nothing else: float64 [1+N+N*N] = {n, mean,
        cov} of an unmasked transfer (vst_cwct_stats_code on a packed code, vst_cwct_stats* on a dense one), or with a static
        plan (plan_masks, learn_slots) [32, 1+N+N*N], a record per label slot (vst_cwct_stats_labels_code /
        vst_cwct_stats_labels).  With `out` it is written there (a ring slot of a video loop); nothing synchronises.
        by_label=True: `plan` is a per-frame plan (plan_frame) on the packed route (max_slots <= 8, N = 32); the records of its
        slots 0 .. max_slots - 1 go to `out` [32, rec] under the plan's own table, in stream order.  Records of two frames then
        line up by label, not by slot: pool_stats(plans=...) is the pool that takes them."""
        B, N, cH, cW = content_feat.shape
        rec = 1 + N + N * N
        if not 0 <= int(b) < B:
            raise ValueError(f"sample {b} of a batch of {B}")
        if plan is None and not by_label:
            packed = self._route_of(content_feat, masked=False) == "packed_rows"
            dev = content_feat.packed.device if packed else content_feat.device
            out = self._check_record_out(out, (rec,), dev)
            if packed:
                return self.stats_code(content_feat, b, out=out)
            return self.stats(self._prep(content_feat).reshape(B, N, -1)[b], out=out)
        if by_label and (plan is None or plan.work is None):
            raise ValueError("by_label lines the records of per-frame plans (plan_frame) up by label: a static plan's slots are "
                             "the same in every frame")
        if plan.work is not None and not by_label:
            raise ValueError("a statistics window needs a static plan (plan_masks): a per-frame plan's slots differ from frame to frame")
        if tuple(content_feat.shape) != plan.content_shape:
            raise ValueError(f"plan was made for a content code of shape {plan.content_shape}, got {tuple(content_feat.shape)}")
        if self.use_double:
            raise NotImplementedError("transfer_with_plan has no fp64 form")
        if by_label and (plan.cm_rows is None or not 1 <= int(plan.max_slots) <= 8 or N != 32
                         or self._route_of(content_feat, masked=True, max_slots=plan.max_slots) != "masked_packed_rows"):
            raise NotImplementedError("by_label needs the packed route: a PackedCode of N = 32 and plan_frame(..., max_slots <= 8)")
        route = self._route_of(content_feat, masked=True, max_slots=plan.max_slots)
        ms, tab = int(plan.max_slots), plan.tables[b]
        if route == "masked_packed_rows":
            dev = content_feat.packed.device
            out = self._check_record_out(out, (self.MAX_SLOTS, rec), dev)
            self._ensure_mask_rows(plan)
            ws = self._workspace(_lib.lib().vst_cwct_stats_labels_code_workspace_bytes(cH, cW), dev)
            _call(dev, "vst_cwct_stats_labels_code", _ptr(content_feat.packed[b]), cH, cW, _ptr(plan.cm_rows[b]), _ptr(tab), ms,
                  _ptr(out), _ptr(ws))
            return out
        if route != "masked_single_pass":
            raise NotImplementedError("transfer_with_plan needs N in (32, 64, 128)")
        c = self._prep(content_feat).reshape(B, N, -1)
        out = self._check_record_out(out, (self.MAX_SLOTS, rec), c.device)
        self._stats_labels(c[b], plan.cm[b], tab, ms, out=out)
        return out

    @staticmethod
    def pool_stats(records, weights=None, decay=1.0, cut=0.0, out=None, used=None, plans=None):
        """The record(s) of a window of frames (vst_cwct_stats_pool): records = the frames' records NEWEST FIRST (frame_stats:
        float64 device tensors [rec] or [R, rec], all of one shape, 1..8 of them), weights = one per age (default decay ** age).
        cut > 0: the first age whose record lies further than cut x tr(C_0) from the newest (|dmu|^2 + |dC|_F) ends the window:
        a scene cut.  A window of one frame, or one that a cut or unusable records (n < 2) reduce to it, is a bit copy.
        out: where to write (same shape, overlapping no input); used: int32 [R] (or [1]), the frames pooled per record.
        plans: one uint8 device tensor of LABEL_PLAN_BYTES per record block [max_slots, rec] - the per-frame plan (plan_frame:
        plan.tables[0]) that frame's records were reduced under (frame_stats(by_label=True)).  The records are then lined up by
        the label their slot holds (vst_cwct_stats_pool_keyed): the result is in the newest plan's slot order, a label an older
        frame does not hold skips that frame, and `used` is [max_slots] with 0 for the slots the newest plan does not use (whose
        records are left unwritten).
        One launch on the current stream; returns the pooled tensor."""
        records = list(records)
        if not 1 <= len(records) <= _lib.STATS_POOL_MAX:
            raise ValueError(f"a window holds 1..{_lib.STATS_POOL_MAX} frames, got {len(records)}")
        r0 = records[0]
        for r in records:
            if not torch.is_tensor(r) or not r.is_cuda or r.dtype != torch.float64 or not r.is_contiguous() or r.dim() not in (1, 2) \
                    or r.shape != r0.shape or r.device != r0.device:
                raise ValueError("records are contiguous float64 tensors [rec] or [R, rec] of one shape on one GPU")
        R, rec = (1, r0.shape[0]) if r0.dim() == 1 else (int(r0.shape[0]), int(r0.shape[1]))
        N = int(round(((4 * rec - 3) ** 0.5 - 1) / 2))
        if 1 + N + N * N != rec:
            raise ValueError(f"a record holds 1 + N + N * N doubles, got {rec}")
        if weights is None:
            decay = float(decay)
            if not 0.0 < decay <= 1.0:
                raise ValueError(f"decay must be in (0, 1], got {decay}")
            weights = [decay ** a for a in range(len(records))]
        weights = [float(w) for w in weights]
        if len(weights) != len(records):
            raise ValueError(f"one weight per frame: {len(weights)} weights for {len(records)} frames")
        if out is None:
            out = torch.empty_like(r0)
        elif not torch.is_tensor(out) or out.dtype != torch.float64 or out.shape != r0.shape or out.device != r0.device \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float64 {tuple(r0.shape)} tensor on {r0.device}")
        if used is not None and (not torch.is_tensor(used) or used.dtype != torch.int32 or used.numel() != R
                                 or used.device != r0.device or not used.is_contiguous()):
            raise ValueError(f"used must be a contiguous int32 [{R}] tensor on {r0.device}")
        ptrs = (C.c_void_p * len(records))(*[r.data_ptr() for r in records])
        w = (C.c_double * len(records))(*weights)
        if plans is not None:
            plans = list(plans)
            if r0.dim() != 2 or len(plans) != len(records):
                raise ValueError(f"plans: one per record block [max_slots, rec], got {len(plans)} for {len(records)} blocks of "
                                 f"shape {tuple(r0.shape)}")
            for t in plans:
                if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.numel() != _lib.LABEL_PLAN_BYTES or t.device != r0.device \
                        or not t.is_contiguous():
                    raise ValueError(f"a plan is a contiguous uint8 tensor of {_lib.LABEL_PLAN_BYTES} bytes on {r0.device}")
            pp = (C.c_void_p * len(plans))(*[t.data_ptr() for t in plans])
            _call(r0.device, "vst_cwct_stats_pool_keyed", ptrs, pp, w, len(records), R, N, float(cut), _ptr(out), _ptr(used))
            return out
        _call(r0.device, "vst_cwct_stats_pool", ptrs, w, len(records), R, N, float(cut), _ptr(out), _ptr(used))
        return out

    def _content_record(self, content_stats, content_feat, plan, b, by_label=False):
        """The content record the factor of a windowed transfer runs on: content_stats(the frame's own record, b).  A callable
        that already holds that record (a video loop that reduced the frame into its ring) says so with a `held(b)` method, and
        it is not computed twice.
        by_label (a per-frame plan): the plan exists only now, inside the transfer, so nobody can hold the record yet.  A
        callable with a `record_out(b)` method offers the [32, rec] buffer the record is to be written to (its ring slot; None
        or no method: a fresh tensor); it is computed once, there, and the call is content_stats(record, b, plan table) - the
        table (uint8 [LABEL_PLAN_BYTES], the frame's own buffer: copy it to keep it) is the key the records line up by."""
        if by_label:
            offer = getattr(content_stats, "record_out", None)
            own = self.frame_stats(content_feat, plan, b, out=offer(b) if offer is not None else None, by_label=True)
            got = content_stats(own, b, plan.tables[b])
        else:
            held = getattr(content_stats, "held", None)
            own = held(b) if held is not None else None
            if own is None:
                own = self.frame_stats(content_feat, plan, b)
            got = content_stats(own, b)
        if not torch.is_tensor(got) or got.dtype != torch.float64 or got.numel() != own.numel() or got.device != own.device \
                or not got.is_contiguous():
            raise ValueError(f"content_stats must return a contiguous float64 tensor of {own.numel()} values on {own.device}")
        return got

    # ------------------------------------------------------------------ reference surface
    def transfer(self, content_feat, style_feat, cmask=None, smask=None, strength=None):
        """models/cWCT.py:18-22.  strength (this repo's extension, on every transfer call): a map at the code's resolution or
        a bind_strength object; the result is x + s (A(x) - x) per code pixel."""
        if cmask is None or smask is None:
            return self._transfer(content_feat, style_feat, strength)
        return self._transfer_seg(content_feat, style_feat, cmask, smask, strength)

    def _transfer(self, content_feat, style_feat, strength=None):
        """models/cWCT.py:24-47, per sample (== interpolation(c,[s],[1.0],0.0))."""
        return self.interpolation(content_feat, [style_feat], [1.0], 0.0, strength=strength)

    def interpolation(self, content_feat, styl_feat_list, alpha_s_list, alpha_c=0.0, cmask=None, smask_list=None, strength=None,
                      style_map=None):
        """models/cWCT.py:206-262.  With label maps (cmask[b], smask_list[i][b]; this repo's extension): per sample and label
        the same mix on the gathered columns, as _transfer_seg (:49-109) gathers them, for the labels that pass
        compute_label_info (:178) against every style map; other pixels keep the content feature.
        style_map (this repo's extension): K weight planes at the code's resolution or a bind_style_map object, in place of
        alpha_s_list (which must then be None): sum_k w_k(p) A_k(x) per code pixel, A_k = the map of style k alone at alpha_c."""
        self.last_style_map = None
        B, N, cH, cW = content_feat.shape
        if style_map is not None:
            if alpha_s_list is not None:
                raise ValueError("a style map takes the place of alpha_s_list: pass None")
            if cmask is not None or smask_list is not None:
                raise ValueError("style maps are not supported on the masked routes")
            smap = self._style_map_of(style_map, content_feat, len(styl_feat_list))
            sm = self._strength_of(strength, content_feat)
            feats = []
            for sf in styl_feat_list:
                assert sf.shape[0] == B and sf.shape[1] == N
                feats.append(sf if isinstance(sf, PackedCode) and not sf.stale and not self.use_double
                             else self._prep(sf).reshape(B, N, -1))
            one = lambda t, b: self.stats_code(t, b) if isinstance(t, PackedCode) else self.stats(t[b])      # noqa: E731
            per_b = [[one(s, b) for s in feats] for b in range(B)]
            return self._transfer_style_map(content_feat, lambda b: per_b[b], smap.K, alpha_c, smap, sm, couple=True)
        self.check_mix(len(styl_feat_list), alpha_s_list)
        sm = self._strength_of(strength, content_feat)
        if cmask is not None or smask_list is not None:
            if cmask is None or smask_list is None:
                raise ValueError("a masked interpolation needs cmask and smask_list")
            self.check_mix(len(styl_feat_list), alpha_s_list, len(smask_list))
            for sf in styl_feat_list:
                assert sf.shape[0] == B and sf.shape[1] == N
            return self._interpolation_seg(content_feat, list(styl_feat_list), [float(a) for a in alpha_s_list], float(alpha_c),
                                           cmask, list(smask_list), mix=True, sm=sm)
        in_dtype = content_feat.dtype
        packed = self._route_of(content_feat, masked=False) == "packed_rows"   # statistics on the packed rows; map applied by the inverse pass
        c = None if packed else self._prep(content_feat).reshape(B, N, -1)
        styles = []
        for sf in styl_feat_list:
            assert sf.shape[0] == B and sf.shape[1] == N
            styles.append(sf if isinstance(sf, PackedCode) and not sf.stale and not self.use_double
                          else self._prep(sf).reshape(B, N, -1))
        one = lambda t, b: self.stats_code(t, b) if isinstance(t, PackedCode) else self.stats(t[b])      # noqa: E731
        stats = [(one(content_feat, b) if packed else self.stats(c[b]), [one(s, b) for s in styles]) for b in range(B)]
        affines, infos = [], []
        for cs, ss in stats:
            affines.append(self.factor(cs, ss, alpha_s_list, alpha_c, N))
            infos.append(self.last_info)
        if B > 1:
            # the reference factors the [B,N,N] stacks at once: if any sample needs jitter, every sample of the batch gets it
            # (cWCT.py:122-128).  Second factor call from the batch maximum of the retry counts (on the device: no host sync).
            need = torch.stack(infos).max(dim=0).values
            need[1] = 0
            affines = [self.factor(cs, ss, alpha_s_list, alpha_c, N, min_tries=need) for cs, ss in stats]
        if packed:
            return content_feat.with_affines(torch.stack(affines), self._strength_rows(sm))
        out = torch.empty_like(c)
        for b in range(B):
            self.apply(c[b], affines[b], out=out[b])
            if sm is not None:
                self._blend(c[b], out[b], sm, b, out[b])
        return out.to(in_dtype).reshape(B, N, cH, cW)

    def _interpolation_seg(self, content_feat, styles, alphas, alpha_c, cmask, smask_list, mix, sm=None):
        """The masked forms of `interpolation` (mix=True) and of `transfer` (mix=False: one style, weight 1, alpha_c = 0)."""
        N = content_feat.shape[1]
        if "masked_per_label" in self._route_of(content_feat, masked=True, mix=mix):
            # no matrix-core form at N = 16 or at the untuned widths, no single-pass fp64 form: one statistics + apply pass per
            # label (cWCT.py:83-103)
            return self._interpolation_seg_per_label(content_feat, styles, alphas, alpha_c, cmask, smask_list, sm)
        plan = self.plan_masks(cmask, smask_list, content_feat.shape, [tuple(sf.shape) for sf in styles], content_feat.device)
        if mix and self._is_packed_code(content_feat) and N == 32 and content_feat.sp_steps == 2:
            # one read-back: a single call may take the packed rows if the slots fit.  (`transfer` never reads a plan back: it
            # is the call of a loop that re-plans every frame, and stays free of synchronisation.)
            self.learn_slots(plan)
        return self.transfer_with_plan(content_feat, styles, plan, alpha_s=alphas if mix else None, alpha_c=alpha_c, strength=sm)

    def _interpolation_seg_per_label(self, content_feat, styles, alphas, alpha_c, cmask, smask_list, sm=None):
        """The per-label form (N = 16, untuned widths, fp64): the reference's loop, with every style's columns gathered."""
        B, N, cH, cW = content_feat.shape
        in_dtype = content_feat.dtype
        c = self._prep(content_feat).reshape(B, N, -1)
        ss = [self._prep(sf).reshape(B, N, -1) for sf in styles]
        out = c.clone()
        up = lambda m: torch.from_numpy(np.ascontiguousarray(m.reshape(-1).astype(np.uint8))).to(c.device)      # noqa: E731
        for b in range(B):
            cm_np = np.asarray(cmask[b])
            sm_np = [np.asarray(sm[b]) for sm in smask_list]
            if cm_np.size != cH * cW or any(m.size != sf.shape[2] * sf.shape[3] for m, sf in zip(sm_np, styles)):
                raise ValueError("masks must have the feature resolution")
            infos = [self.compute_label_info(cm_np, m) for m in sm_np]
            cm, sms = up(cm_np), [up(m) for m in sm_np]
            for label in infos[0][0]:
                if not all(ind[label] for _, ind in infos):
                    continue
                affine = self.factor(self.stats(c[b], cm, int(label)), [self.stats(s[b], m, int(label)) for s, m in zip(ss, sms)],
                                     alphas, alpha_c, N)
                self.apply(c[b], affine, out=out[b], mask=cm, label=int(label))
            if sm is not None:                           # (pixels no label took hold x in out: they keep it)
                self._blend(c[b], out[b], sm, b, out[b])
        return out.to(in_dtype).reshape(B, N, cH, cW)

    # ------------------------------------------------------------------ cached-style extension
    def style_stats(self, style_feat):
        """Per-sample statistics of a style code [B,N,sH,sW] -> list of B stats tensors.  The reference
        re-encodes and re-factors the style for every frame (video_transfer.py:195); a video loop can
        compute this once per style and call transfer_with_stats per frame."""
        B, N = style_feat.shape[:2]
        packed = isinstance(style_feat, PackedCode) and not style_feat.stale and not self.use_double
        s = None if packed else self._prep(style_feat).reshape(B, N, -1)
        out = []
        for b in range(B):
            st = self.stats_code(style_feat, b) if packed else self.stats(s[b])
            if self.use_double:                      # (the prefactored record stores an fp32 factor)
                out.append(st)
                continue
            info = torch.zeros(1, dtype=torch.int32, device=st.device)
            work = ()
            if self._family(N):                      # the width-generic Cholesky works in the factor's workspace
                fws = torch.empty(_lib.lib().vst_cwct_factor_n_workspace_bytes(N), dtype=torch.uint8, device=st.device)
                work = (_ptr(fws), fws.numel())
            # Cholesky once per style, in place
            _call(st.device, "vst_cwct_prefactor" + self._family(N), _ptr(st), N, float(self.eps), _ptr(st), _ptr(info), *work)
            out.append(st)
        return out

    def transfer_with_stats(self, content_feat, style_stats, alpha_c=0.0, inplace=False, alpha_s=None, strength=None,
                            style_map=None, content_stats=None):
        """transfer(content, style) with the style side given as style_stats(style) (len B or 1).  inplace=True
        overwrites a contiguous fp32 content code instead of allocating the result (like the reference's masked path,
        cWCT.py:62,103; one 128 MiB buffer less per 1024x1024 frame in flight).  Several styles: style_stats = a list of K such
        lists and alpha_s = their K weights (default: equal), mixed per sample like interpolation.  strength: as in transfer;
        an in-place call then applies out of place and blends into the content code.  style_map: as in interpolation, with
        style_stats the list of K lists; alpha_s must then be None and the result is a new tensor.
        content_stats: a callable f(record, b) -> record (the statistics window of a video loop): it is called on the frame's own
        content record (frame_stats) and the factor runs on what it returns, e.g. pool_stats over a ring of records."""
        self.last_style_map = None
        B, N, cH, cW = content_feat.shape
        sm = self._strength_of(strength, content_feat)
        if len(style_stats) and isinstance(style_stats[0], (list, tuple)):
            per_style = [list(st) for st in style_stats]
        else:
            per_style = [list(style_stats)]
        if style_map is not None:
            if alpha_s is not None:
                raise ValueError("a style map takes the place of alpha_s: pass None")
            smap = self._style_map_of(style_map, content_feat, len(per_style))
            return self._transfer_style_map(content_feat, lambda b: [st[b if len(st) > 1 else 0] for st in per_style], smap.K,
                                            alpha_c, smap, sm, couple=False, content_stats=content_stats)
        alphas = [1.0 / len(per_style)] * len(per_style) if alpha_s is None else [float(a) for a in alpha_s]
        if len(per_style) == 1 and alpha_s is None:
            alphas = [1.0]
        self.check_mix(len(per_style), alphas)
        pick = lambda b: [st[b if len(st) > 1 else 0] for st in per_style]      # noqa: E731
        if content_stats is not None:
            own = lambda b, x2d: self._content_record(content_stats, content_feat, None, b)      # noqa: E731
        else:
            own = lambda b, x2d: self.stats_code(content_feat, b) if x2d is None else self.stats(x2d)      # noqa: E731
        if self._route_of(content_feat, masked=False) == "packed_rows":   # nothing is written here, the inverse pass applies the map
            affines = [self.factor(own(b, None), pick(b), alphas, alpha_c, N) for b in range(B)]
            return content_feat.with_affines(torch.stack(affines), self._strength_rows(sm))
        in_dtype = content_feat.dtype
        c = self._prep(content_feat).reshape(B, N, -1)
        out = c if inplace and not isinstance(content_feat, PackedCode) and c.data_ptr() == content_feat.data_ptr() else torch.empty_like(c)
        for b in range(B):
            affine = self.factor(own(b, c[b]), pick(b), alphas, alpha_c, N)
            if sm is None:
                self.apply(c[b], affine, out=out[b])
            else:                                        # the blend needs x and A(x): never applied in place
                y = self.apply(c[b], affine, out=None if out is c else out[b])
                self._blend(c[b], y, sm, b, out[b])
        return out.to(in_dtype).reshape(B, N, cH, cW)

    def _transfer_seg(self, content_feat, style_feat, cmask, smask, strength=None):
        """models/cWCT.py:49-109: the masked interpolation of one style with weight 1 and alpha_c = 0."""
        return self._interpolation_seg(content_feat, [style_feat], [1.0], 0.0, cmask, [smask], mix=False,
                                       sm=self._strength_of(strength, content_feat))

    # ------------------------------------------------------------------ single-pass masked transfer
    # Everything `_transfer_seg` derives from the label maps (models/cWCT.py:72-76,166-189) happens on the device: the
    # histograms (vst_label_hist per map), the validity rule and a label -> slot table (vst_label_plan_hists); then ONE
    # statistics pass per code for all labels, one factor launch (a workgroup per label) and ONE apply pass.  No host histogram,
    # no per-label launches, no synchronisation: a per-frame mask costs its upload (or nothing, if it is already a device
    # tensor).  One style or several (the masked interpolation) is the same code: a plan's style side is a list.
    MAX_SLOTS = 32

    def _mask_to_device(self, m, hw, device, what):
        H, W = hw
        if torch.is_tensor(m):
            if m.numel() != H * W:
                raise ValueError(f"masks must have the feature resolution ({what} {tuple(m.shape)} vs {(H, W)})")
            return m.to(device=device, dtype=torch.uint8).reshape(-1).contiguous()
        m_np = np.asarray(m)
        if self.resize_masks and m_np.shape != (H, W):
            m_np = self.resize(np.ascontiguousarray(m_np.astype(np.uint8)), H, W)
        if m_np.size != H * W:
            raise ValueError(f"masks must have the feature resolution ({what} {m_np.shape} vs {(H, W)})")
        if m_np.dtype != np.uint8 and (m_np.max() > 255 or m_np.min() < 0):
            raise ValueError("labels must be in [0, 255]")
        return torch.from_numpy(np.ascontiguousarray(m_np.reshape(-1).astype(np.uint8))).to(device, non_blocking=True)

    @staticmethod
    def _plan_hists(hist_c, lut, style_hists, cap, table, flags=None):
        """vst_label_plan_hists: the label -> slot table (at most `cap` slots) of a content histogram, remapped through `lut`
        if given, against every style histogram; an overflow is raised in `flags` if given."""
        hp = (C.c_void_p * len(style_hists))(*[h.data_ptr() for h in style_hists])
        _call(table.device, "vst_label_plan_hists", _ptr(hist_c), _ptr(lut), hp, len(style_hists), int(cap), _ptr(table), _ptr(flags))
        return table

    @staticmethod
    def _plan_maps(cm, sms):
        """The table of one content map against its style maps (flat uint8 device tensors), all MAX_SLOTS slots: one
        vst_label_hist per map, then _plan_hists."""
        hists = torch.empty((1 + len(sms), 256), dtype=torch.int32, device=cm.device)
        for j, m in enumerate([cm] + list(sms)):
            _call(cm.device, "vst_label_hist", _ptr(m), m.numel(), _ptr(hists[j]))
        table = torch.empty(_lib.LABEL_PLAN_BYTES, dtype=torch.uint8, device=cm.device)
        return cWCT._plan_hists(hists[0], None, list(hists[1:]), cWCT.MAX_SLOTS, table)

    def plan_masks(self, cmask, smask, content_shape, style_shape, device):
        """Device-side label plan per sample (numpy label maps as the reference hands them over, or uint8 device tensors).
        A video loop whose masks do not change builds this once; one whose masks change per frame pays the small histogram
        and plan kernels per frame and no host work beyond the upload.  Several styles: smask = a list of per-style maps
        (smask[i][b]) and style_shape = the list of their codes' shapes; a label then needs to be valid against every style."""
        B, N, cH, cW = content_shape
        if len(style_shape) and isinstance(style_shape[0], (int, np.integer)):      # one style: one shape, one stack of maps
            smask, style_shape = [smask], [style_shape]
        if N not in (32, 64, 128):
            raise NotImplementedError("the single-pass masked transfer needs N in (32, 64, 128)")
        if not 1 <= len(style_shape) <= _lib.MAX_STYLES or len(smask) != len(style_shape):
            raise ValueError(f"1..{_lib.MAX_STYLES} styles with one label map each, got {len(style_shape)} shapes and "
                             f"{len(smask)} maps")
        plan = MaskPlan(content_shape, style_shape)      # max_slots = 0: learn_slots() tightens it
        for b in range(B):
            cm = self._mask_to_device(cmask[b], (cH, cW), device, "content")
            sms = [self._mask_to_device(sm[b], shape[2:], device, "style") for sm, shape in zip(smask, plan.style_shapes)]
            plan.cm.append(cm)
            for per_style, m in zip(plan.sms, sms):
                per_style.append(m)
            plan.tables.append(self._plan_maps(cm, sms))
        return plan

    @staticmethod
    def plan_info(plan, b=0):
        """(labels with a slot, overflow flag) of sample b — synchronises; for tests and diagnostics."""
        raw = plan.tables[b].cpu().numpy()
        n, over = int(raw[:4].view(np.int32)[0]), int(raw[4:8].view(np.int32)[0])
        return [int(v) for v in raw[8 + 2048 + 256: 8 + 2048 + 256 + n]], bool(over)

    def learn_slots(self, plan):
        """Read the slot counts back once (one synchronisation) so that later launches cover only the slots in use — worth
        it for a plan that is reused over a clip."""
        plan.max_slots = max(1, max(len(self.plan_info(plan, b)[0]) for b in range(len(plan.tables))))
        self._ensure_mask_rows(plan)
        return plan

    @staticmethod
    def _mask_rows(mask, H, W):
        """A flat uint8 [H * W] device label map in a PackedCode's row order (vst_mask_to_code)."""
        rows = torch.empty_like(mask)
        _call(mask.device, "vst_mask_to_code", _ptr(mask), _ptr(rows), H, W)
        return rows

    def _ensure_mask_rows(self, plan):
        """The content label maps in a PackedCode's row order, for plans the packed masked route can take (photorealistic
        codes, at most 8 slots).  Built HERE, once, and completed before returning: the plan is then shared by frames in
        flight on several streams (FramePipeline, bench.py), none of which may meet a half-written map."""
        B, N, cH, cW = plan.content_shape
        if plan.cm_rows is not None or N != 32 or not (1 <= int(plan.max_slots) <= 8):
            return
        dev = plan.cm[0].device
        with torch.cuda.device(dev):
            rows_all = [self._mask_rows(plan.cm[b], cH, cW) for b in range(B)]
            torch.cuda.current_stream(dev).synchronize()
        plan.cm_rows = rows_all

    def _stats_labels(self, x2d, mask, table, max_slots, out=None):
        N, Lp = x2d.shape
        if out is None:
            out = torch.empty(self.MAX_SLOTS * (1 + N + N * N), dtype=torch.float64, device=x2d.device)
        ws = self._workspace(_lib.lib().vst_cwct_labels_workspace_bytes(N, Lp), x2d.device)
        _call(x2d.device, "vst_cwct_stats_labels", _ptr(x2d), N, Lp, _ptr(mask), _ptr(table), int(max_slots), _ptr(out), _ptr(ws))
        return out

    def _prefactor_labels(self, stats, table, max_slots, N):
        """Per-slot records -> prefactored, in place (vst_cwct_prefactor_labels): the factor then reads the stored Cholesky
        factor back exactly, so the affines keep their bits and a bound style costs no Cholesky per frame."""
        info = torch.empty(self.MAX_SLOTS, dtype=torch.int32, device=stats.device)
        _call(stats.device, "vst_cwct_prefactor_labels", _ptr(stats), _ptr(table), int(max_slots), N, float(self.eps), _ptr(stats),
              _ptr(info))
        return stats

    def bind_style(self, plan, style_feat, prefactor=True):
        """Per-label statistics of the style code (or of every style code of a multi-style plan: a list), computed and factored
        once (the masked counterpart of style_stats): transfer_with_plan then skips the style side for every later frame.
        Rebind when a style code changes.  prefactor=False keeps the raw {n, mean, cov} records (same affines, bit for bit)."""
        feats = list(style_feat) if isinstance(style_feat, (list, tuple)) else [style_feat]
        if len(feats) != len(plan.style_shapes):
            raise ValueError(f"plan was made for {len(plan.style_shapes)} style(s), got {len(feats)}")
        styles = []
        for sf, shape, sm in zip(feats, plan.style_shapes, plan.sms):
            B, N = sf.shape[:2]
            if tuple(sf.shape) != shape:
                raise ValueError(f"plan was made for a style code of shape {shape}, got {tuple(sf.shape)}")
            s = self._prep(sf).reshape(B, N, -1)
            recs = [self._stats_labels(s[b], sm[b], plan.tables[b], plan.max_slots) for b in range(B)]
            if prefactor:
                recs = [self._prefactor_labels(r, plan.tables[b], plan.max_slots, N) for b, r in enumerate(recs)]
            styles.append(recs)
        plan.styles = styles
        return plan

    # ------------------------------------------------------------------ per-frame masks (vstnet_amd/masks.py, csrc/masks.hip)
    def bind_style_labels(self, style_code, style_seg, prefactor=True):
        """Style binding keyed by label, computed once per style (and style map): `style_seg` is the [sH,sW] label map (numpy or
        a uint8 device tensor; self-remap it first if the frames' maps are remapped).  One image.  Lists of codes and maps give a
        list of bindings (plan_frame takes it).  The records are prefactored (prefactor=False: raw, same affines bit for bit)."""
        if isinstance(style_code, (list, tuple)):
            if len(style_code) != len(style_seg) or not 1 <= len(style_code) <= _lib.MAX_STYLES:
                raise ValueError(f"1..{_lib.MAX_STYLES} styles with one label map each")
            return [self.bind_style_labels(zc, sg, prefactor) for zc, sg in zip(style_code, style_seg)]
        B, N, sH, sW = style_code.shape
        if B != 1 or N not in (32, 64, 128):
            raise NotImplementedError("bind_style_labels takes one style code with N in (32, 64, 128)")
        if self.use_double:
            raise NotImplementedError("the per-frame masked transfer has no fp64 form")
        dev = style_code.device
        s = self._prep(style_code).reshape(B, N, -1)
        sm = self._mask_to_device(style_seg[0] if not torch.is_tensor(style_seg) and np.asarray(style_seg).ndim == 3 else style_seg,
                                  (sH, sW), dev, "style")
        hist = torch.empty(256, dtype=torch.int32, device=dev)
        _call(dev, "vst_label_hist", _ptr(sm), sm.numel(), _ptr(hist))
        tab = torch.empty(_lib.LABEL_PLAN_BYTES, dtype=torch.uint8, device=dev)
        self._plan_hists(hist, None, [hist], self.MAX_SLOTS, tab)        # the style map against itself
        stats = self._stats_labels(s[0], sm, tab, 0)
        return StyleBinding(style_code.shape, hist, tab, self._prefactor_labels(stats, tab, 0, N) if prefactor else stats)

    @staticmethod
    def frame_buffers(H, W, N, device):
        """What one frame's plan writes: a ring slot of the frame loop owns one set (nothing is allocated per frame)."""
        return {"rows": torch.empty(H * W, dtype=torch.uint8, device=device),
                "labels": torch.empty(H * W, dtype=torch.uint8, device=device),
                "hist": torch.empty(256, dtype=torch.int32, device=device),
                "lut": torch.empty(256, dtype=torch.uint8, device=device),
                "plan": torch.empty(_lib.LABEL_PLAN_BYTES, dtype=torch.uint8, device=device),
                "flags": torch.zeros(1, dtype=torch.int32, device=device),
                "cs": torch.empty(cWCT.MAX_SLOTS * (1 + N + N * N), dtype=torch.float64, device=device),
                "affines": torch.empty(cWCT.MAX_SLOTS * (N * N + N), dtype=torch.float32, device=device),
                "info": torch.empty(cWCT.MAX_SLOTS * (2 + _lib.MAX_STYLES), dtype=torch.int32, device=device)}

    def plan_frame(self, mask_dev, binding, remap=None, colours=False, max_slots=8, buffers=None, flags=None, N=32):
        """A MaskPlan for ONE frame from its uploaded map, built entirely in stream order: `mask_dev` = uint8 device tensor
        [H,W] (labels) or, with colours=True, [H,W,3] (dictionary colours); `remap` = a masks.DeviceSegReMapping (self +
        cross remapping against the binding's style map) or None.  max_slots = 8 (the packed route's cap, set WITHOUT a
        read-back): the plan takes `masked_packed_rows` on a PackedCode; max_slots = 32: the dense route (the image-order
        labels are made as well).  More valid labels than the cap raise VST_MASK_OVERFLOW in `plan.flags`, a label outside
        the relation table VST_MASK_OUT_OF_TABLE; the caller looks at the word when the frame retires.  The plan lives on the
        current stream: its buffers (`buffers`, from frame_buffers) must stay untouched until the frame's work is done.
        `binding` may be a list of bindings (bind_style_labels of several styles): a label then needs to be valid against every
        style map, and the cross remapping looks at the labels every style map holds."""
        bindings = list(binding) if isinstance(binding, (list, tuple)) else [binding]
        if not 1 <= len(bindings) <= _lib.MAX_STYLES:
            raise ValueError(f"1..{_lib.MAX_STYLES} style bindings, got {len(bindings)}")
        if not torch.is_tensor(mask_dev) or not mask_dev.is_cuda or mask_dev.dtype != torch.uint8:
            raise ValueError("plan_frame takes a uint8 tensor on the GPU")
        if mask_dev.dim() != (3 if colours else 2) or (colours and mask_dev.shape[2] != 3):
            raise ValueError(f"expected {'[H,W,3]' if colours else '[H,W]'}, got {tuple(mask_dev.shape)}")
        if not 1 <= int(max_slots) <= self.MAX_SLOTS:
            raise ValueError("max_slots must be in 1..32")
        if self.use_double:
            raise NotImplementedError("the per-frame masked transfer has no fp64 form")
        H, W = int(mask_dev.shape[0]), int(mask_dev.shape[1])
        if any(bd.shape[1] != N for bd in bindings) or N not in (32, 64, 128):
            raise ValueError(f"the style binding was made for N = {bindings[0].shape[1]}")
        dev = mask_dev.device
        mask_dev = mask_dev.contiguous()
        buf = buffers if buffers is not None else self.frame_buffers(H, W, N, dev)
        if buf["rows"].numel() != H * W:
            raise ValueError("buffers were made for another frame size")
        fl = flags if flags is not None else buf["flags"]
        packed = int(max_slots) <= 8 and N == 32
        plan = MaskPlan((1, N, H, W), [bd.shape for bd in bindings])
        with torch.cuda.device(dev):
            fl.zero_()
            if packed:        # the one pass over the map: labels in the code's row order + histogram
                _call(dev, "vst_mask_prepare", _ptr(mask_dev), int(bool(colours)), H, W, _ptr(buf["rows"]), _ptr(buf["hist"]))
                plan.cm, plan.cm_rows = [None], [buf["rows"]]
            else:
                labels = mask_dev.reshape(-1)
                if colours:
                    labels = buf["labels"]
                    _call(dev, "vst_colors_to_labels", _ptr(mask_dev), _ptr(labels), H * W)
                _call(dev, "vst_label_hist", _ptr(labels), H * W, _ptr(buf["hist"]))
                plan.cm = [labels]
            lut = None
            if remap is not None:
                lut = remap.lut(buf["hist"], H * W, style_hist=self._common_hist(bindings), out=buf["lut"], flags=fl)
            self._plan_hists(buf["hist"], lut, [bd.hist for bd in bindings], max_slots, buf["plan"], fl)
        plan.sms = [[None] for _ in bindings]        # (the style maps live in the bindings)
        plan.tables = [buf["plan"]]
        plan.max_slots = int(max_slots)
        plan.bindings, plan.flags, plan.work = bindings, fl, buf
        return plan

    def _common_hist(self, bindings):
        """Per label the smallest count over the bindings' style maps (made once per set of bindings): what the cross remapping
        of a frame's map looks at, so that a remapped label is one every style map holds."""
        if len(bindings) == 1:
            return bindings[0].hist
        key = tuple(id(bd) for bd in bindings)
        cache = getattr(self, "_hist_cache", None)
        if cache is None or cache[0] != key:
            self._hist_cache = cache = (key, torch.stack([bd.hist for bd in bindings]).min(dim=0).values.contiguous(), bindings)
        return cache[1]

    def _factor_labels(self, cs, records, table, style_plans, alphas, alpha_c, max_slots, N, affines, info):
        """vst_cwct_factor_labels_mix, the one factor call of every masked form: per slot of `table` the affine map from the
        content records `cs` and one record block per style (`records`), mixed with `alphas` and `alpha_c`.  The blocks are in
        the table's slot order, or (style_plans: one table per style) keyed by label through each style's own plan.  The plain
        transfer is one style with weight 1 and alpha_c = 0."""
        K = len(records)
        sp = (C.c_void_p * K)(*[r.data_ptr() for r in records])
        pp = (C.c_void_p * K)(*[p.data_ptr() for p in style_plans]) if style_plans is not None else None
        al = (C.c_float * K)(*alphas)
        _call(cs.device, "vst_cwct_factor_labels_mix", _ptr(cs), sp, pp, al, K, float(alpha_c), _ptr(table), int(max_slots),
              float(self.eps), N, _ptr(affines), _ptr(info))

    def _apply_labels(self, x2d, out, affines, mask, table, max_slots):
        """vst_cwct_apply_labels: every pixel of the [N,L] code through the affine map of its label's slot, one pass."""
        N, Lp = x2d.shape
        _call(x2d.device, "vst_cwct_apply_labels", _ptr(x2d), _ptr(out), N, Lp, _ptr(affines), _ptr(mask), _ptr(table), int(max_slots),
              _lib.PRECISIONS[self.precision])

    def _mix_of(self, plan, alpha_s, alpha_c):
        """(weights, alpha_c, mix) of a transfer_with_plan call.  mix = False: the plain transfer (one style, no weights given,
        alpha_c = 0); it is computed as the mix [1.0], 0.0 and differs in the route's name only."""
        K = len(plan.style_shapes)
        alpha_c = float(alpha_c)
        if not 0.0 <= alpha_c <= 1.0:
            raise ValueError(f"alpha_c must be in [0, 1], got {alpha_c}")
        if alpha_s is None:
            return [1.0 / K] * K, alpha_c, not (K == 1 and alpha_c == 0.0)
        alphas = [float(a) for a in alpha_s]
        if len(alphas) != K:
            raise ValueError(f"the plan has {K} style(s), got {len(alphas)} weights")
        return alphas, alpha_c, True

    def _style_codes(self, plan, style_feat, B, N):
        """The style codes a plan without bound styles needs, as [B,N,L] tensors (one per style)."""
        feats = list(style_feat) if isinstance(style_feat, (list, tuple)) else [style_feat]
        if len(feats) != len(plan.style_shapes) or any(f is None or tuple(f.shape) != sh for f, sh in zip(feats, plan.style_shapes)):
            raise ValueError("transfer_with_plan needs the style code the plan was made for (or bind_style first)")
        return [self._prep(f).reshape(B, N, -1) for f in feats]

    def _style_records(self, plan, b, s, max_slots):
        """One per-slot record block per style for sample b: a per-frame plan's bindings, the bound styles, or the statistics
        of the style codes `s` under the plan's style maps."""
        if plan.bindings is not None:
            return [bd.stats for bd in plan.bindings]
        if plan.styles is not None:
            return [st[b] for st in plan.styles]
        return [self._stats_labels(si[b], sm[b], plan.tables[b], max_slots) for si, sm in zip(s, plan.sms)]

    def transfer_with_plan(self, content_feat, style_feat, plan, inplace=False, alpha_s=None, alpha_c=0.0, strength=None,
                           content_stats=None, by_label=False):
        """transfer(content, style, cmask, smask) with the mask work given as plan_masks(...) (and, after bind_style,
        the style side too; style_feat may then be None).  Pixels whose label has no slot keep the content feature.
        alpha_s / alpha_c (per call: one binding serves a clip whose mix changes every frame) make it the masked
        interpolation: alpha_s = one weight per style of the plan (default: equal weights; a plan of several styles takes a list
        of style codes unless they are bound).
        On a PackedCode (photorealistic codes, at most 8 label slots, known after learn_slots) the per-label statistics run on
        the packed rows with the label map in the rows' order (made once per plan), and the result is the same rows with the
        per-row maps pending - the inverse pass applies them while it loads its state.  strength: as in transfer (pixels
        whose label has no slot keep the content feature whatever their strength).
        content_stats: as in transfer_with_stats, on the [32, rec] block of per-slot records; static plans only (the slots of
        a per-frame plan differ from frame to frame: ValueError) - unless by_label=True: the frame's records are then reduced
        under the per-frame plan (packed route only) and content_stats(record, b, plan table) lines them up by label
        (_content_record has the protocol; pool_stats(plans=...) is the pool)."""
        B, N, cH, cW = content_feat.shape
        if content_stats is not None and plan.work is not None and not by_label:
            raise ValueError("content_stats needs a static plan (plan_masks): a per-frame plan's slots differ from frame to frame")
        if by_label and (content_stats is None or plan.work is None):
            raise ValueError("by_label goes with content_stats and a per-frame plan (plan_frame)")
        sm = self._strength_of(strength, content_feat)
        if tuple(content_feat.shape) != plan.content_shape:
            raise ValueError(f"plan was made for a content code of shape {plan.content_shape}, got {tuple(content_feat.shape)}")
        if self.use_double:
            raise NotImplementedError("transfer_with_plan (this repo's cached-mask extension) has no fp64 form: with "
                                      "use_double=True call transfer(content, style, cmask, smask)")
        alphas, alpha_c, mix = self._mix_of(plan, alpha_s, alpha_c)
        route = self._route_of(content_feat, masked=True, max_slots=plan.max_slots, mix=mix)
        packed = route.endswith("masked_packed_rows")
        if not packed and not route.endswith("masked_single_pass"):
            raise NotImplementedError("transfer_with_plan needs N in (32, 64, 128)")
        ms, K = int(plan.max_slots), len(plan.style_shapes)
        s = None
        if plan.styles is None and plan.bindings is None:
            s = self._style_codes(plan, style_feat, B, N)
        style_plans = [bd.plan for bd in plan.bindings] if plan.bindings is not None else None
        if packed:
            dev = content_feat.packed.device
            self._ensure_mask_rows(plan)          # (a plan whose max_slots was set by hand: built and completed now)
            ws = self._workspace(_lib.lib().vst_cwct_stats_labels_code_workspace_bytes(cH, cW), dev)
            per_image = []
        else:
            if plan.cm[0] is None:
                raise ValueError("this per-frame plan was made for the packed route (max_slots <= 8): plan_frame(..., max_slots=32) "
                                 "makes the one a dense code takes")
            in_dtype = content_feat.dtype
            c = self._prep(content_feat).reshape(B, N, -1)
            dev = c.device
            out = c if inplace and not isinstance(content_feat, PackedCode) and c.data_ptr() == content_feat.data_ptr() else torch.empty_like(c)
        for b in range(B):
            tab = plan.tables[b]
            if packed and plan.work is not None:         # a per-frame plan: the frame's ring slot owns these
                cs, affines, info = plan.work["cs"], plan.work["affines"], plan.work["info"]
                if info.numel() < self.MAX_SLOTS * (2 + K):
                    raise ValueError("the frame's buffers are too small for this many styles: make them with frame_buffers")
            else:
                cs = torch.empty(self.MAX_SLOTS * (1 + N + N * N), dtype=torch.float64, device=dev) if packed else None
                affines = torch.empty(self.MAX_SLOTS * (N * N + N), dtype=torch.float32, device=dev)
                info = torch.empty(self.MAX_SLOTS * (2 + K), dtype=torch.int32, device=dev)
            if content_stats is not None:
                cs = self._content_record(content_stats, content_feat, plan, b, by_label)
            elif packed:
                _call(dev, "vst_cwct_stats_labels_code", _ptr(content_feat.packed[b]), cH, cW, _ptr(plan.cm_rows[b]), _ptr(tab), ms,
                      _ptr(cs), _ptr(ws))
            else:                                        # (the dense statistics allocate their own records)
                cs = self._stats_labels(c[b], plan.cm[b], tab, ms)
            self._factor_labels(cs, self._style_records(plan, b, s, ms), tab, style_plans, alphas, alpha_c, ms, N, affines, info)
            self.last_info = info
            if packed:
                per_image.append((affines, plan.cm_rows[b], tab))
            elif sm is None:
                self._apply_labels(c[b], out[b], affines, plan.cm[b], tab, ms)
            else:                                        # the blend needs x and A(x): never applied in place
                y = torch.empty_like(c[b]) if out is c else out[b]
                self._apply_labels(c[b], y, affines, plan.cm[b], tab, ms)
                self._blend(c[b], y, sm, b, out[b])
        if packed:
            return content_feat.with_label_affines(per_image, ms, self._strength_rows(sm))
        return out.to(in_dtype).reshape(B, N, cH, cW)

    # ------------------------------------------------------------------ helpers (public by convention)
    def cholesky_dec(self, conv, invert=False):
        """models/cWCT.py:111-132 for one [N,N] matrix (1 <= N <= 256)."""
        N = conv.shape[-1]
        dev = conv.device
        st = torch.zeros(1 + N + N * N, dtype=torch.float64, device=dev)
        st[0] = 2.0
        st[1 + N:] = conv.detach().double().reshape(-1)
        ident = self._identity_stats(N, dev)
        if invert:      # T = I * L^-1
            aff = self.factor(st, [ident], [1.0], 0.0, N)
        else:           # T = L * I^-1
            aff = self.factor(ident, [st], [1.0], 0.0, N)
        return aff[: N * N].reshape(N, N).to(conv.dtype)

    def whitening(self, x):
        """models/cWCT.py:134-149 on a 2-D [N,L] matrix."""
        x = self._prep(x)
        N = x.shape[0]
        aff = self.factor(self.stats(x), [self._identity_stats(N, x.device)], [1.0], 0.0, N)
        return self.apply(x, aff)

    def coloring(self, content_whiten_feat, style_feat):
        """models/cWCT.py:152-164 on 2-D matrices."""
        w = self._prep(content_whiten_feat)
        s = self._prep(style_feat)
        N = w.shape[0]
        aff = self.factor(self._identity_stats(N, w.device), [self.stats(s)], [1.0], 0.0, N)
        return self.apply(w, aff)

    def compute_label_info(self, content_seg, style_seg):
        """models/cWCT.py:166-189 (histograms instead of one np.where per label; same result)."""
        content_seg, style_seg = np.asarray(content_seg), np.asarray(style_seg)
        if content_seg.size == 0 or style_seg.size == 0:
            return
        max_label = int(np.max(content_seg)) + 1
        ch = np.bincount(content_seg.reshape(-1).astype(np.int64), minlength=max_label)
        sh = np.bincount(style_seg.reshape(-1).astype(np.int64), minlength=max_label)
        label_set = np.nonzero(ch)[0].astype(content_seg.dtype)
        label_indicator = np.zeros(max_label)
        for l in label_set:
            a, b = int(ch[l]), int(sh[l])
            label_indicator[l] = a > 10 and b > 10 and a / b < 100 and b / a < 100
        return label_set, label_indicator

    def resize(self, img, H, W):
        """models/cWCT.py:191-197 (NEAREST)."""
        from PIL import Image
        if len(img.shape) == 2:
            return np.array(Image.fromarray(img).resize((W, H), Image.NEAREST))
        return np.array(Image.fromarray(img, mode='RGB').resize((W, H), Image.NEAREST))

    def get_index(self, feat, label):
        """models/cWCT.py:199-204."""
        mask = np.where(feat.reshape(feat.shape[0] * feat.shape[1]) == label)
        if mask[0].size <= 0:
            return None
        return torch.LongTensor(mask[0])

from . import cwct_ops as ops  # noqa: E402,F401  (vstnet_amd.cwct.ops: the kernels one by one, for tests and tools)
