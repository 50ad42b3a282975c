"""csrc/layout.hip restated in numpy with integer and bit operations only, from the layout comments of layout.hip, common.h
(PackedConvLayout) and include/vstnet.h: the packed conv weights byte for byte, the uint8 frame edge, and vst_normalize_block.
No kernel result went into anything here; tests/test_layout_host.py checks the statements against each other on the CPU,
tests/test_gpu_layout.py holds the card to them."""
import numpy as np

# ------------------------------------------------------------------------------------------- packed conv weights
# (cout, cin): the nine shapes of the published net; odd cout padded to 16 and no conv3 section; conv3 section with three
# K chunks and cout not a multiple of 64
PACK_SHAPES = ((4, 16), (4, 4), (16, 4), (16, 64), (16, 16), (64, 16), (64, 256), (64, 64), (256, 64), (5, 32), (80, 96))
SECTIONS = ("f32", "bf16_hi", "bf16_lo", "f16_conv3", "f16")


def pack_layout(cout, cin):
    """common.h, packed_conv_layout: byte offset and length of every section (f16_conv3 has length 0 off the stage-3 shapes)"""
    ksteps = 9 * (cin // 32) if cin >= 32 else (5 if cin == 16 else 2)
    coutp = (cout + 15) // 16 * 16
    f32_used = 9 * cin * cout * 4
    f32_bytes = (f32_used + 255) // 256 * 256
    frag = ksteps * 4 * coutp * 16
    sp = frag if (cin >= 64 and cout >= 64) else 0
    off = {"f32": (0, f32_bytes), "bf16_hi": (f32_bytes, frag), "bf16_lo": (f32_bytes + frag, frag),
           "f16_conv3": (f32_bytes + 2 * frag, sp), "f16": (f32_bytes + 2 * frag + sp, frag)}
    return {"ksteps": ksteps, "coutp": coutp, "f32_used": f32_used, "sections": off, "total": f32_bytes + 3 * frag + sp}


def bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even on the bit pattern (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def f16_bits(x):
    """float32 -> fp16 bit patterns, round to nearest even, overflow to +-Inf (what the device's _Float16 cast does)"""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def k_coords(cin, ksteps, conv3=False):
    """(tap, ci) of fragment element (ks, kg, j), each int array [ksteps, 4, 8]: the three K orders of the MFMA kernels and,
    conv3=True, the permuted order of conv3.hip ({4 kg + r, 16 + 4 kg + r} of the 32-channel chunk)"""
    ks = np.arange(ksteps)[:, None, None]
    kg = np.arange(4)[None, :, None]
    j = np.arange(8)[None, None, :]
    if cin >= 32:
        tap = ks % 9 + 0 * kg + 0 * j
        ci = (ks // 9) * 32 + ((j >> 2) * 16 + kg * 4 + (j & 3) if conv3 else kg * 8 + j)
    elif cin == 16:
        tap = 2 * ks + (kg >> 1) + 0 * j
        ci = (kg & 1) * 8 + j + 0 * ks
    else:
        tap = 8 * ks + 2 * kg + (j >> 2)
        ci = (j & 3) + 0 * ks + 0 * kg
    return tap, ci


def fragment_values(w, conv3=False, coords=None):
    """the float32 value of every fragment element, [ksteps, 4, coutp, 8]; taps > 8 and co >= cout are zero"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, cin = w.shape[:2]
    L = pack_layout(cout, cin)
    tap, ci = coords if coords is not None else k_coords(cin, L["ksteps"], conv3)
    ok = (tap < 9) & (ci < cin)
    w9 = w.reshape(cout, cin, 9)
    g = w9[:, np.where(ok, ci, 0), np.where(ok, tap, 0)]                  # [cout, ksteps, 4, 8]
    g = np.where(ok[None], g, np.float32(0))
    out = np.zeros((L["ksteps"], 4, L["coutp"], 8), np.float32)
    out[:, :, :cout, :] = g.transpose(1, 2, 0, 3)
    return out


def packed_sections(w, coords=None):
    """every section of vst_pack_conv's buffer as bytes, by name"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, cin = w.shape[:2]
    L = pack_layout(cout, cin)
    f32 = np.zeros(L["sections"]["f32"][1], np.uint8)
    f32[:L["f32_used"]] = np.ascontiguousarray(w.reshape(cout, cin, 9).transpose(2, 1, 0)).view(np.uint8).ravel()   # [tap][ci][co]
    v = fragment_values(w, coords=coords)
    hi = bf16_bits(v)
    lo = bf16_bits(v - bf16_value(hi))                                  # the subtraction in float32
    sec = {"f32": f32.tobytes(), "bf16_hi": hi.tobytes(), "bf16_lo": lo.tobytes(), "f16": f16_bits(v).tobytes(), "f16_conv3": b""}
    if L["sections"]["f16_conv3"][1]:
        sec["f16_conv3"] = f16_bits(fragment_values(w, conv3=True)).tobytes()
    return sec


def packed_conv(w_oihw):
    """the whole buffer vst_pack_conv writes for an OIHW float32 tensor (the unspecified bytes as zeros)"""
    sec = packed_sections(w_oihw)
    return b"".join(sec[name] for name in SECTIONS)


def specified_mask(cout, cin):
    """False on the bytes between 9 cin cout 4 and the 256-rounded end of the fp32 section: the kernel does not write them"""
    L = pack_layout(cout, cin)
    m = np.ones(L["total"], bool)
    m[L["f32_used"]:L["sections"]["f32"][1]] = False
    return m


def packed_mismatches(got, want, cout, cin):
    """{section: number of differing specified bytes}, empty when the two buffers agree; the comparison both tests use"""
    L = pack_layout(cout, cin)
    g, w_ = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    assert g.size == w_.size == L["total"], (g.size, w_.size, L["total"])
    bad = (g != w_) & specified_mask(cout, cin)
    out = {}
    for name in SECTIONS:
        o, n = L["sections"][name]
        if bad[o:o + n].any():
            out[name] = int(bad[o:o + n].sum())
    return out


F32 = np.float32
# planted weights: signed zeros, the fp16 limits, two bf16 ties that go to even in opposite directions (1 + 2^-8 down to 1,
# 1 + 3 2^-8 up to 1 + 2^-6), a value below the fp16 normals that fp16 still holds exactly, and two values whose lo term
# (2^-10 (1 + 2^-8), 2^-10 (1 + 2^-7 + 2^-8)) is itself a bf16 tie, again one each way
PLANTED = np.array([0.0, -0.0, 65504.0, -65504.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -20,
                    1 + 2.0 ** -10 + 2.0 ** -18, 1 + 2.0 ** -10 + 2.0 ** -17 + 2.0 ** -18], F32)


def pack_weights(cout, cin, seed=0):
    """seeded normals times a per-row logspace(-3, 3), PLANTED written over seeded positions; max |w| is exactly 65504"""
    rng = np.random.default_rng([seed, cout, cin])
    w = rng.standard_normal((cout, cin, 3, 3)) * np.logspace(-3, 3, cout)[:, None, None, None]
    w = w.astype(F32)
    assert np.abs(w).max() < 65504
    w.reshape(-1)[rng.choice(w.size, PLANTED.size, replace=False)] = PLANTED
    return w


# ------------------------------------------------------------------------------------------- uint8 frame edge
U8_SHAPES = ((1, 8, 8), (2, 12, 68), (1, 8, 132))        # a 64-wide tile that ends mid-row; a full tile + 4; two tiles + 4; B > 1


def u8_frames(B, H, W):
    """[B, H, W, 3] uint8: 7 is coprime to 256, so any 256 consecutive pixels hold every byte value in every channel position"""
    p = np.arange(B * H * W, dtype=np.int64).reshape(B, H, W, 1)
    return ((p * 7 + np.arange(3) * 85 + 3) % 256).astype(np.uint8)


def u8_to_unit(u8):
    """transforms.ToTensor: a true float32 division"""
    return u8.astype(F32) / F32(255)


def unit_to_u8(x, rounding=False):
    """mul(255).clamp(0, 255).byte(): truncation toward zero of the float32 product, NaN -> 0 stated here, not left to a cast"""
    t = np.ascontiguousarray(x, dtype=F32) * F32(255)
    nan = np.isnan(t)
    t = np.clip(np.where(nan, F32(0), t), F32(0), F32(255))
    t = np.floor(t + F32(0.5)) if rounding else np.trunc(t)
    return t.astype(np.uint8)


def u8_edge_values():
    """the float32 values whose quantisation is pinned: the specials, then k / 255 with its two float32 neighbours for all k"""
    k = np.arange(256, dtype=F32) / F32(255)
    fam = np.stack([k, np.nextafter(k, F32(2)), np.nextafter(k, F32(-1))], 1).ravel()
    special = np.array([-0.0, -1e-7, -3.0, 1.0, np.nextafter(F32(1), F32(2)), 7.5, np.inf, -np.inf, np.nan], F32)
    return np.concatenate([special, fam]).astype(F32)


def u8_edge_planes(B, H, W):
    """[B, 3, H, W] float32 filled with u8_edge_values() in turn: the specials first, then the k / 255 family in a seeded order
    (a frame with fewer places than values holds all the specials and a sample of the family)"""
    v = u8_edge_values()
    n_special = v.size - 768
    order = np.concatenate([np.arange(n_special), n_special + np.random.default_rng(7).permutation(768)])
    n = B * 3 * H * W
    return v[order[np.arange(n) % v.size]].reshape(B, 3, H, W)


# ------------------------------------------------------------------------------------------- vst_normalize_block
NORM_CASES = ((4, 4, 16), (16, 1, 4), (64, 16, 64), (256, 64, 256))      # (cin1, mid, cout)
NORM_SEED = 0
HALF_BAND = 1e-4


def row_log2_norms(w):
    """log2 of the fp64 L2 norm of every row of an OIHW float32 tensor; -inf for a zero row, inf / nan kept"""
    r = np.ascontiguousarray(w, dtype=F32).astype(np.float64).reshape(w.shape[0], -1)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return np.log2(np.sqrt((r * r).sum(1)))


def pow2_scales(w, round_down=False):
    """(scales float32 [rows], in_band bool [rows]): 2^-round(log2 norm), the exponent clamped to +-40, 1 for a zero or
    non-finite norm; in_band marks rows whose log2 norm is within HALF_BAND of a half-integer (the device sums the squares
    in float32 in another order, so such a row may round either way).  Domain: rows whose sum of squares fits float32; the
    device takes the norm from a float32 sum, which past 2^128 is +Inf and gives scale 1."""
    lg = row_log2_norms(w)
    live = np.isfinite(lg)
    lgl = np.where(live, lg, 0.0)
    r = np.floor(lgl) if round_down else np.floor(lgl + 0.5)
    r = np.clip(r, -40, 40)
    s = np.where(live, np.ldexp(1.0, -r.astype(np.int64)), 1.0).astype(F32)
    band = live & (np.abs(lgl - np.floor(lgl) - 0.5) < HALF_BAND)
    return s, band


def normalize_block(w1, b1, w4, b4, w7, round_down=False):
    """the five tensors after vst_normalize_block, the scales {s1, s2} and the rows in the half-integer band, every product and
    quotient in float32 in the kernel's order (powers of two: exact short of over- and underflow)"""
    w1, b1, w4, b4, w7 = (np.array(t, dtype=F32) for t in (w1, b1, w4, b4, w7))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s1, band1 = pow2_scales(w1, round_down)
        w1 = w1 * s1[:, None, None, None]
        b1 = b1 * s1
        w4 = w4 / s1[None, :, None, None]
        s2, band2 = pow2_scales(w4, round_down)
        w4 = w4 * s2[:, None, None, None]
        b4 = b4 * s2
        w7 = w7 / s2[None, :, None, None]
    return (w1, b1, w4, b4, w7), np.concatenate([s1, s2]), np.concatenate([band1, band2])


def norm_tensors(cin1, mid, cout, seed=NORM_SEED):
    """a block whose row norms span 2^-50 .. 2^50 in both intermediates (both exponent clamps act), with, for mid >= 4, an
    all-zero row and a row holding +Inf in each.  W4 carries the first phase's scales on its columns, so that the rows the second
    phase measures have the chosen magnitudes and no square leaves float32's range."""
    rng = np.random.default_rng([seed, cin1, mid, cout])

    def mag(few):
        """row magnitudes: a permutation of 2^linspace(-50, 50, mid); with 1 or 4 rows, the given exponents"""
        e = rng.permutation(np.round(np.linspace(-50, 50, mid)).astype(np.int64))
        return np.ldexp(1.0, np.array(few[mid]) if mid in few else e)[:, None, None, None]

    w1 = (rng.standard_normal((mid, cin1, 3, 3)) * mag({1: [45], 4: [50, 0, 0, -3]})).astype(F32)
    if mid >= 4:
        w1[1] = 0
        w1[2, cin1 // 2, 1, 2] = np.inf
    s1, _ = pow2_scales(w1)
    w4 = (rng.standard_normal((mid, mid, 3, 3)) * mag({1: [-45], 4: [0, -50, 7, 0]})).astype(F32) * s1[None, :, None, None]
    if mid >= 4:
        w4[0] = 0
        w4[3, mid - 1, 0, 0] = np.inf
    b1 = (rng.standard_normal(mid) * 4).astype(F32)
    b4 = (rng.standard_normal(mid) * 4).astype(F32)
    w7 = rng.standard_normal((cout, mid, 3, 3)).astype(F32)
    return w1, b1, w4, b4, w7
