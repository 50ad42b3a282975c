"""Ultra-resolution stylisation: halo-tiled passes for frames of any size.

RevResNet is fully convolutional with a finite receptive field, and the cWCT needs only the global {n, mean, cov} statistics of
the content and the style codes.  So a frame of any size is stylised in tiles whose interiors partition it: a tile's output
interior is computed from a window (interior + halo, clipped at the image border) that holds everything the interior depends
on, and the statistics of the interiors merge into the whole frame's.  Device memory is bounded by the window, not the frame.

  pass S : encode the style windows (halo R_f), statistics of their interiors (vst_cwct_stats_code_rect), merged
  pass 1 : the same for the content
  factor : once, from the merged records (alpha_c: vst_cwct_factor; masks: cWCT's label plan of the FULL masks and its
           factor call, vst_cwct_factor_labels_mix)
  pass 2 : encode every content window with halo R_f + R_i, attach the affine map, decode, keep the interior

R_f / R_i = receptive_radius(net, "forward" / "inverse"), derived from the architecture ("Ultra-resolution").
Frames and outputs stay on the host; a window's uint8 pixels cross the bus once per pass.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .code import PackedCode, from_dense
from .cwct import _call, _ptr, _stream_ptr, cWCT  # noqa: F401  (the masked steps are the driver's own helpers)

ALIGN = 4                       # H, W, tile origins and sizes: multiples of the frame alignment (down_scale)
# device bytes per window pixel of a pass-2 window: pass workspace (288) + packed code (128) + the materialised code or a float
# frame (128, NCHW routes) + the uint8 window and its output (6)
WINDOW_BYTES_PER_PX = 288 + 128 + 128 + 6


def max_frame_pixels() -> int:
    """H * W of the largest frame the whole-frame passes take (include/vstnet.h VST_MAX_FRAME_PIXELS)."""
    return int(_lib.lib().vst_max_frame_pixels())


# ------------------------------------------------------------------------------------------------ receptive radius
def _blocks(net):
    """(stride, kernel) of every coupling block of the passes in forward order: the stack, then channel_reduction."""
    if getattr(net, "_generic", False):
        raise NotImplementedError("tiled stylisation supports the two published architectures (photorealistic and artistic); "
                                  "a generic-architecture RevResNet (csrc/generic.hip) has no derived receptive radius")
    blocks = list(net.stack) + list(net.channel_reduction.block_list)
    return [(int(b.stride), int(b.conv[1].kernel_size[0])) for b in blocks]


def _conv(iv, stride, pad):
    """Outputs of a (2 pad + 1)-tap conv of `stride` that read an input of the interval iv (None = nothing)."""
    if iv is None:
        return None
    a, b = iv
    return (-((pad - a) // stride), (b + pad) // stride)


def _residual(iv, stride, kernel):
    """residual_block.conv (models/RevResNet.py:79-88): conv(stride), conv, conv."""
    pad = (kernel - 1) // 2
    return _conv(_conv(_conv(iv, stride, pad), 1, pad), 1, pad)


def _hull(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return (min(a[0], b[0]), max(a[1], b[1]))


def _squeeze(iv):
    return None if iv is None else (iv[0] >> 1, iv[1] >> 1)


def _unsqueeze(iv):
    return None if iv is None else (2 * iv[0], 2 * iv[1] + 1)


def _cone_forward(blocks, p):
    """Frame pixel p (one axis) -> the frame-pixel span of the code pixels it reaches (models/RevResNet.py:96-104, :210-223)."""
    x1, x2 = (p, p), None              # inj_pad + split: the image's channels are in the first half, the second is zero
    for s, k in blocks:
        f = _residual(x2, s, k)
        if s == 2:
            x1, x2 = _squeeze(x1), _squeeze(x2)
        x1, x2 = x2, _hull(f, x1)
    scale = 2 ** sum(s == 2 for s, _ in blocks)
    q = _hull(x1, x2)                  # merge (+ spread: a cell of the coarsest level is scale x scale frame pixels)
    return q[0] * scale, q[1] * scale + scale - 1


def _cone_inverse(blocks, c, sp_steps):
    """Code pixel c (one axis) -> the frame pixels the inverse pass derives from it (models/RevResNet.py:106-116, :225-239)."""
    q = c >> sp_steps                  # un-spread: sp_steps squeezes; a code pixel's channels are in both halves
    state = ((q, q), (q, q))
    for s, k in reversed(blocks):
        x2, y1 = state
        if s == 2:
            x2 = _unsqueeze(x2)
        x1 = _hull(_residual(x2, s, k), y1)
        if s == 2:
            x1 = _unsqueeze(x1)
        state = (x1, x2)
    return state[0]                    # the frame is the first channels of the first half (inj_pad.inverse)


def receptive_radius(net, direction: str) -> int:
    """Influence radius in frame pixels of ``forward`` (frame -> code) or ``inverse`` (code -> frame): a change of one frame
    pixel (one code pixel) leaves every code pixel (frame pixel) farther than this along either axis bit-for-bit unchanged.
    The exact cone of the architecture over every alignment of the changed pixel, rounded up to the frame alignment."""
    blocks = _blocks(net)
    scale = 2 ** sum(s == 2 for s, _ in blocks)
    sp = int(net.sp_steps)
    foot = scale >> sp                 # frame pixels per code pixel along an axis (1: photorealistic, 2: artistic)
    if direction not in ("forward", "inverse"):
        raise ValueError("direction must be 'forward' or 'inverse'")
    r = 0
    for p in range(64, 64 + 4 * scale):
        if direction == "forward":
            lo, hi = _cone_forward(blocks, p)
            r = max(r, p - lo, hi - p)
        else:
            lo, hi = _cone_inverse(blocks, p, sp)
            r = max(r, p * foot - lo, hi - (p * foot + foot - 1))
    return -(-r // ALIGN) * ALIGN


# ------------------------------------------------------------------------------------------------ tile plan
class Tile(NamedTuple):
    """Interior [iy0, iy1) x [ix0, ix1) and window [wy0, wy1) x [wx0, wx1) in frame pixels."""
    iy0: int
    iy1: int
    ix0: int
    ix1: int
    wy0: int
    wy1: int
    wx0: int
    wx1: int

    @property
    def window_hw(self):
        return self.wy1 - self.wy0, self.wx1 - self.wx0

    @property
    def rect(self):
        """The interior in window coordinates: (y0, x0, h, w)."""
        return self.iy0 - self.wy0, self.ix0 - self.wx0, self.iy1 - self.iy0, self.ix1 - self.ix0


def _split(n, tile):
    """Edges of ceil(n / tile) intervals of [0, n): multiples of ALIGN, at least 2 ALIGN long, as equal as possible."""
    units = n // ALIGN
    k = max(1, min(-(-n // tile), units // 2))
    base, extra = divmod(units, k)
    edges = [0]
    for i in range(k):
        edges.append(edges[-1] + (base + (1 if i < extra else 0)) * ALIGN)
    return edges


def tile_plan(H: int, W: int, tile: int, halo: int, max_pixels: int = None):
    """Tiles whose interiors partition the H x W frame (at most tile x tile each) and whose windows are the interiors grown by
    `halo` on every side and clipped at the image border - there the window's border is the frame's, so the reflection padding
    applies exactly where the whole-frame pass applies it.  Raises if a window exceeds max_pixels (default: the guard)."""
    if H % ALIGN or W % ALIGN or H < 2 * ALIGN or W < 2 * ALIGN:
        raise ValueError(f"H and W must be multiples of {ALIGN} and >= {2 * ALIGN} (got {H}x{W})")
    if tile < 2 * ALIGN or halo < 0 or halo % ALIGN:
        raise ValueError(f"tile must be >= {2 * ALIGN} and halo a non-negative multiple of {ALIGN} (got {tile}, {halo})")
    max_pixels = max_frame_pixels() if max_pixels is None else int(max_pixels)
    ys, xs = _split(H, tile), _split(W, tile)
    tiles = []
    for y0, y1 in zip(ys[:-1], ys[1:]):
        for x0, x1 in zip(xs[:-1], xs[1:]):
            t = Tile(y0, y1, x0, x1, max(0, y0 - halo), min(H, y1 + halo), max(0, x0 - halo), min(W, x1 + halo))
            h, w = t.window_hw
            if h * w > max_pixels:
                raise ValueError(f"a {h}x{w} window exceeds the whole-frame limit of {max_pixels} pixels: use a smaller tile")
            tiles.append(t)
    return tiles


def default_tile(halo: int, budget_bytes: int, max_pixels: int = None) -> int:
    """Largest multiple of 512 whose window (tile + 2 halo)^2 is within the guard and the device-memory budget (at least 512)."""
    max_pixels = max_frame_pixels() if max_pixels is None else int(max_pixels)
    t = 512
    while True:
        w = t + 512 + 2 * halo
        if w * w > max_pixels or w * w * WINDOW_BYTES_PER_PX > budget_bytes:
            return t
        t += 512


def needs_tiling(H: int, W: int, budget_bytes: int, max_pixels: int = None) -> bool:
    """True if a frame is past the whole-frame guard or its whole-frame working set does not fit the memory budget."""
    max_pixels = max_frame_pixels() if max_pixels is None else int(max_pixels)
    return H * W > max_pixels or H * W * WINDOW_BYTES_PER_PX > budget_bytes


def memory_budget(device=None) -> int:
    """Device bytes the tiled driver plans with: half of what is free now."""
    free, _ = torch.cuda.mem_get_info(device)
    return int(free) // 2


# ------------------------------------------------------------------------------------------------ statistics merge
def merge_stats(records, N: int):
    """Combine {n, mean, cov} records (fp64 tensors [..., 1 + N + N*N] of disjoint pixel sets; a leading slot axis is kept) into
    the record of their union: Chan et al.'s pairwise formula on n, mean and M2 = cov (n - 1), where parts with n <= 1 add no
    co-moment of their own (their cov is 0/0)."""
    R = torch.stack([r.to(torch.float64) for r in records])
    n = R[..., 0]
    mean = R[..., 1:1 + N]
    cov = R[..., 1 + N:].reshape(*R.shape[:-1], N, N)
    nt = n.sum(0)
    mu = (n[..., None] * mean).sum(0) / torch.where(nt > 0, nt, torch.ones_like(nt))[..., None]
    own = torch.where((n > 1)[..., None, None], cov * (n - 1)[..., None, None], torch.zeros_like(cov))
    d = mean - mu
    m2 = own.sum(0) + (n[..., None, None] * d[..., :, None] * d[..., None, :]).sum(0)
    covm = m2 / (nt - 1)[..., None, None]
    return torch.cat([nt[..., None], mu, covm.reshape(*covm.shape[:-2], N * N)], dim=-1)


# ------------------------------------------------------------------------------------------------ device helpers
def stats_code_rect(cwct, code, H, W, sp_steps, rect):
    """{n, mean, cov} of the rows of ONE image's packed code (flat float32) whose pixels lie in rect = (y0, x0, h, w)."""
    N = 32 if sp_steps == 2 else 128
    out = torch.empty(1 + N + N * N, dtype=torch.float64, device=code.device)
    ws = cwct._workspace(_lib.lib().vst_cwct_stats_code_workspace_bytes(H, W, sp_steps), code.device)
    _call(code.device, "vst_cwct_stats_code_rect", _ptr(code), H, W, sp_steps, *[int(v) for v in rect], _ptr(out), _ptr(ws))
    return out


def stats_labels_code_rect(cwct, code, H, W, rect, mask_rows, plan, max_slots):
    """Per-slot records [32, 1 + 32 + 32*32] of the rows of ONE photorealistic packed code inside rect = (y0, x0, h, w)."""
    N = 32
    out = torch.empty(cwct.MAX_SLOTS, 1 + N + N * N, dtype=torch.float64, device=code.device)
    ws = cwct._workspace(_lib.lib().vst_cwct_stats_labels_code_workspace_bytes(H, W), code.device)
    _call(code.device, "vst_cwct_stats_labels_code_rect", _ptr(code), H, W, *[int(v) for v in rect], _ptr(mask_rows), _ptr(plan),
          int(max_slots), _ptr(out), _ptr(ws))
    return out


def mask_rows(mask_u8_dev, H, W):
    """An [H, W] uint8 label map (device, flat) in the packed code's row order: the step cWCT.plan_masks' plans take per map."""
    return cWCT._mask_rows(mask_u8_dev, H, W)


def label_plan(cmask_dev, smask_dev):
    """cWCT.plan_masks' table of two flat uint8 device label maps -> (plan buffer, number of slots)."""
    plan = cWCT._plan_maps(cmask_dev, [smask_dev])
    return plan, int(plan[:4].cpu().numpy().view(np.int32)[0])


def _host_u8(img, what):
    a = np.asarray(img)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"{what} must be a host uint8 array [H,W,3] (got {a.dtype} {a.shape})")
    return a


def _host_labels(seg, hw, what):
    a = np.asarray(seg)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.shape != tuple(hw):
        raise ValueError(f"{what} must be a label map of the image's size {tuple(hw)} (got {a.shape})")
    if a.dtype != np.uint8 and (a.max() > 255 or a.min() < 0):
        raise ValueError("labels must be in [0, 255]")
    return np.ascontiguousarray(a.astype(np.uint8))


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ drivers
def _one_style(style_u8):
    if isinstance(style_u8, (list, tuple)):
        raise ValueError("several styles in tiled mode are out of scope: the tiled drivers take one style image")


def _no_style_map(style_map):
    if style_map is not None:
        raise ValueError("style maps in tiled mode are out of scope: the tiled drivers take one style image and no style map")


def stylize_whole(net, cwct, content_u8, style_u8, content_seg=None, style_seg=None, alpha_c=None, preserve_luminance=False,
                  out_float=False, interpolate_labels=False, style_map=None):
    """The whole-frame path (image_transfer.py's stylize) on host arrays: uint8 [H,W,3], or float32 [H,W,3] with out_float.
    interpolate_labels: with masks, alpha_c is applied per label (cWCT.interpolation with label maps) instead of ignored."""
    from .color import luminance_transfer
    _one_style(style_u8)
    _no_style_map(style_map)
    dev = next(net.parameters()).device
    content, style = _host_u8(content_u8, "content"), _host_u8(style_u8, "style")
    masked = content_seg is not None and style_seg is not None
    with torch.no_grad(), torch.cuda.device(dev):
        xc = _to_dev(content, dev)[None]
        z_c = net.forward_u8(xc)
        z_s = net.forward_u8(_to_dev(style, dev)[None])
        if alpha_c is not None and not masked:
            z_cs = cwct.interpolation(z_c, styl_feat_list=[z_s], alpha_s_list=[1.0], alpha_c=alpha_c)
        elif masked and interpolate_labels and alpha_c is not None:
            z_cs = cwct.interpolation(z_c, [z_s], [1.0], alpha_c, _host_labels(content_seg, content.shape[:2], "content_seg")[None],
                                      [_host_labels(style_seg, style.shape[:2], "style_seg")[None]])
        elif masked:
            z_cs = cwct.transfer(z_c, z_s, _host_labels(content_seg, content.shape[:2], "content_seg")[None],
                                 _host_labels(style_seg, style.shape[:2], "style_seg")[None])
        else:
            z_cs = cwct.transfer(z_c, z_s)
        if not preserve_luminance and not out_float:
            return net.inverse_u8(z_cs)[0].cpu().numpy()
        y = net(z_cs, forward=False)
        if preserve_luminance:
            y = luminance_transfer(xc.permute(0, 3, 1, 2).float().div(255.0), y)
        if out_float:
            return y[0].permute(1, 2, 0).contiguous().cpu().numpy()
        return y[0].mul(255.0).clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy()


# How the statistics and the pass-2 apply run on a window's code (names as in cWCT.ROUTES)
TILED_ROUTES = {
    "packed_rows": "unmasked: vst_cwct_stats_code_rect on each window's packed rows; the map is applied by the decode",
    "masked_packed_rows": "masked photorealistic, 1..8 label slots: vst_cwct_stats_labels_code_rect with the window's mask rows; "
                          "per-row maps applied by vst_revnet_decode_labels",
    "masked_single_pass": "masked photorealistic, more than 8 slots: the interior of the materialised window code copied to a "
                          "contiguous buffer for vst_cwct_stats_labels; vst_cwct_apply_labels on the window's code",
    "dense_f64": "use_double, unmasked: the interior of the materialised window code for vst_cwct_stats_f64; "
                 "vst_cwct_apply_f64 on the window's code",
}


def tiled_route(sp_steps, masked, n_slots, use_double):
    if masked and (sp_steps != 2 or use_double):
        raise NotImplementedError("tiled masked stylisation supports photorealistic codes without use_double")
    if use_double:
        return "dense_f64"
    if masked:
        return "masked_packed_rows" if n_slots <= 8 else "masked_single_pass"
    return "packed_rows"


def _encode(net, window_u8, dev):
    z = net.forward_u8(_to_dev(window_u8, dev)[None])
    return z if isinstance(z, PackedCode) else from_dense(z)


def _interior_dense(z, t, sp):
    """The interior of a window's materialised NCHW code as a contiguous [N, pixels] matrix."""
    y0, x0, h, w = t.rect
    f = 1 if sp == 2 else 2
    zi = z.materialize()[0, :, y0 // f:(y0 + h) // f, x0 // f:(x0 + w) // f]
    return zi.reshape(zi.shape[0], -1).contiguous()


def _interior_stats(net, cwct, img, seg, tiles, route, sp, plan, max_slots, dev):
    """Merged statistics of the interiors of `tiles` of one image (pass S / pass 1)."""
    N = 32 if sp == 2 else 128
    recs = []
    for t in tiles:
        h, w = t.window_hw
        z = _encode(net, img[t.wy0:t.wy1, t.wx0:t.wx1], dev)
        if route == "packed_rows":
            recs.append(stats_code_rect(cwct, z.packed[0], h, w, sp, t.rect))
        elif route == "masked_packed_rows":
            rows = mask_rows(_to_dev(seg[t.wy0:t.wy1, t.wx0:t.wx1], dev).reshape(-1), h, w)
            recs.append(stats_labels_code_rect(cwct, z.packed[0], h, w, t.rect, rows, plan, max_slots))
        elif route == "masked_single_pass":
            m = _to_dev(seg[t.iy0:t.iy1, t.ix0:t.ix1], dev).reshape(-1)
            recs.append(cwct._stats_labels(_interior_dense(z, t, sp), m, plan, max_slots).reshape(cwct.MAX_SLOTS, -1))
        else:
            recs.append(cwct.stats(_interior_dense(z, t, sp)))
        del z
    if len(recs) == 1 and tiles[0].rect == (0, 0) + tiles[0].window_hw:
        return recs[0]                  # one tile, the whole image: the record itself
    return merge_stats(recs, N)


def stylize_tiled(net, cwct, content_u8, style_u8, content_seg=None, style_seg=None, alpha_c=None, preserve_luminance=False,
                  tile=None, out_float=False, info=None, interpolate_labels=False, style_map=None):
    """Stylise a host uint8 [H,W,3] content frame of any size with a host uint8 [sH,sW,3] style image (masks: host label maps
    of the images' sizes) in halo tiles of at most tile x tile interior pixels (default: from the guard and the free device
    memory); returns a host uint8 [H,W,3] array, float32 with out_float.  Equal to the whole-frame path up to fp32 noise; a
    tile that covers both images takes the whole-frame path itself (stylize_whole).  `info` (a dict, optional) receives the
    plan, the route and the merged statistics and affine map.  interpolate_labels: with masks, alpha_c is applied per label
    (one style; the factor call of the merged records takes it) instead of ignored."""
    from .color import luminance_transfer
    _one_style(style_u8)
    _no_style_map(style_map)
    content, style = _host_u8(content_u8, "content"), _host_u8(style_u8, "style")
    H, W = content.shape[:2]
    sH, sW = style.shape[:2]
    masked = content_seg is not None and style_seg is not None
    dev = next(net.parameters()).device
    r_f, r_i = receptive_radius(net, "forward"), receptive_radius(net, "inverse")
    limit = max_frame_pixels()
    if tile is None:
        tile = default_tile(r_f + r_i, memory_budget(dev), limit)
    if tile >= max(H, W, sH, sW) and H * W <= limit and sH * sW <= limit:
        if info is not None:
            info.update(route="whole_frame", tile=tile, tiles=1, radius=(r_f, r_i))
        return stylize_whole(net, cwct, content, style, content_seg, style_seg, alpha_c, preserve_luminance, out_float,
                             interpolate_labels)
    cseg = _host_labels(content_seg, (H, W), "content_seg") if masked else None
    sseg = _host_labels(style_seg, (sH, sW), "style_seg") if masked else None
    s_tiles = tile_plan(sH, sW, tile, r_f, limit)
    c1_tiles = tile_plan(H, W, tile, r_f, limit)
    c2_tiles = tile_plan(H, W, tile, r_f + r_i, limit)
    sp = int(net.sp_steps)
    N = 32 if sp == 2 else 128
    L = _lib.lib()
    with torch.no_grad(), torch.cuda.device(dev):
        plan, n_slots = None, 0
        if masked:                      # from the FULL maps: the reference's validity rule sees the global label counts
            plan, n_slots = label_plan(_to_dev(cseg, dev).reshape(-1), _to_dev(sseg, dev).reshape(-1))
        route = tiled_route(sp, masked, n_slots, cwct.use_double)
        ms = max(1, n_slots)
        # the pass workspace of the largest window, once: growing it window by window would hold two at the peak
        net._get_workspace(max(L.vst_pass_workspace_bytes(1, *t.window_hw) for t in s_tiles + c2_tiles), dev)
        ss = _interior_stats(net, cwct, style, sseg, s_tiles, route, sp, plan, ms, dev)
        cs = _interior_stats(net, cwct, content, cseg, c1_tiles, route, sp, plan, ms, dev)
        if masked:
            affine = torch.empty(cwct.MAX_SLOTS * (N * N + N), dtype=torch.float32, device=dev)
            finfo = torch.empty(cwct.MAX_SLOTS * 3, dtype=torch.int32, device=dev)
            csf, ssf = cs.reshape(-1).contiguous(), ss.reshape(-1).contiguous()
            mix_c = float(alpha_c) if interpolate_labels and alpha_c is not None else 0.0      # (without the keyword: ignored)
            cwct._factor_labels(csf, [ssf], plan, None, [1.0], mix_c, ms, N, affine, finfo)
            cwct.last_info = finfo
        else:
            affine = cwct.factor(cs, [ss], [1.0], 0.0 if alpha_c is None else float(alpha_c), N)
        cwct.last_route = route
        out = np.empty((H, W, 3), dtype=np.float32 if out_float else np.uint8)
        for t in c2_tiles:
            h, w = t.window_hw
            y0, x0, ih, iw = t.rect
            z = _encode(net, content[t.wy0:t.wy1, t.wx0:t.wx1], dev)
            if route == "packed_rows":
                zt = z.with_affines(affine[None])
            elif route == "masked_packed_rows":
                rows = mask_rows(_to_dev(cseg[t.wy0:t.wy1, t.wx0:t.wx1], dev).reshape(-1), h, w)
                zt = z.with_label_affines([(affine, rows, plan)], ms)
            elif route == "masked_single_pass":
                zd = z.materialize()
                m = _to_dev(cseg[t.wy0:t.wy1, t.wx0:t.wx1], dev).reshape(-1)
                zt = torch.empty_like(zd)
                cwct._apply_labels(zd[0].view(N, h * w), zt[0].view(N, h * w), affine, m, plan, ms)
            else:
                zd = z.materialize()
                zt = cwct.apply(zd[0].reshape(N, -1), affine).reshape(zd.shape)
            del z
            zd = None
            if not preserve_luminance and not out_float:
                out[t.iy0:t.iy1, t.ix0:t.ix1] = net.inverse_u8(zt)[0, y0:y0 + ih, x0:x0 + iw].cpu().numpy()
                del zt
                continue
            y = net(zt, forward=False)[:, :, y0:y0 + ih, x0:x0 + iw].contiguous()
            del zt
            if preserve_luminance:
                xc = _to_dev(content[t.iy0:t.iy1, t.ix0:t.ix1], dev)[None]
                y = luminance_transfer(xc.permute(0, 3, 1, 2).float().div(255.0), y)
            if out_float:
                out[t.iy0:t.iy1, t.ix0:t.ix1] = y[0].permute(1, 2, 0).cpu().numpy()
            else:
                out[t.iy0:t.iy1, t.ix0:t.ix1] = y[0].mul(255.0).clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy()
    if info is not None:
        info.update(route=route, tile=tile, tiles=len(c2_tiles), radius=(r_f, r_i), content_stats=cs, style_stats=ss,
                    affine=affine, plan=plan, max_slots=ms)
    return out
