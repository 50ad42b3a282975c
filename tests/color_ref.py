"""The Lab luminance blend of csrc/color.hip (`luminance_px`) restated in numpy, three times over one statement of the
operations (helpers of test_color_host.py / test_gpu_color.py):

``Bound``   float64 values that carry a first-order bound on what an fp32 evaluation of the same operations may be off by,
            split as ``A + P * Bp``: ``A`` collects the roundings of ``+ - * /`` (half an ulp each, ``U = 2^-24`` relative,
            whether or not the compiler contracts ``a * b + c`` into an fma: an fma's error is below the two roundings counted
            here) and ``Bp`` the roundings of ``powf`` in units of ``U * |z|``, so that ``P`` is the error of the device's
            ``powf`` in those units and a test can solve for the smallest ``P`` that passes;
``Plain``   the same operations in one numpy dtype with no error terms: ``longdouble`` (the twin that shows float64 is wide
            enough to be the reference) and ``float32`` (an emulation of the kernel, which the planted faults are applied to).

The constants are the kernel's, as their float32 values.  Each of the four selects (sRGB decode at 0.04045, Lab f at 0.008856,
its inverse at 0.2068966, sRGB encode at 0.0031308) records where its argument lies within the argument's own error bound of
the threshold: there either branch is a legitimate fp32 result, so ``reference`` returns one variant per subset of the select
kinds that have such elements (up to 16), flipped on those elements, and an element passes if it is within the bound of any
variant.  A clamp passes its operand's bound through, and drops it where the operand is beyond the limit by more than its bound.
"""
import itertools

import numpy as np

U = 2.0 ** -24                       # half an ulp, relative: one rounding of + - * / to float32
FLOOR = 2.0 ** -126                  # a rounding near zero (flushed or gradual underflow) is absolute, not relative
P_ASSERT = 2.0                       # the powf error the tests assert with, in units of U * |z| (which P stands, and why)
KINDS = ("srgb", "lab_f", "lab_finv", "out")


def c32(x):
    """a constant as the float32 the kernel holds, as a Python float"""
    return float(np.float32(x))


# the constants of color.hip:9-55; `fault` names of test_color_host.py replace single entries
K = {
    "srgb_knee": c32(0.04045), "srgb_a": c32(0.055), "srgb_d": c32(1.055), "gamma": c32(2.4), "srgb_lin": c32(12.92),
    "lab_knee": c32(0.008856), "third": c32(1.0 / 3.0), "lab_m": c32(7.787), "lab_o": c32(16.0 / 116.0),
    "finv_knee": c32(0.2068966), "finv_m": c32(7.787), "out_knee": c32(0.0031308), "inv_gamma": c32(1.0 / 2.4),
    "out_m": c32(1.055), "out_a": c32(0.055), "out_lin": c32(12.92),
    "xyz": [[c32(0.412453), c32(0.357580), c32(0.180423)],
            [c32(0.212671), c32(0.715160), c32(0.072169)],
            [c32(0.019334), c32(0.119193), c32(0.950227)]],
    "xn": c32(0.95047), "zn": c32(1.08883), "xn_inv": c32(0.95047), "zn_inv": c32(1.08883),
    "rgb": [[c32(3.24048134), -c32(1.53715152), -c32(0.49853633)],
            [-c32(0.96925495), c32(1.87599), c32(0.04155593)],
            [c32(0.05564664), -c32(0.20404134), c32(1.05731107)]],
}


# ------------------------------------------------------------------------------------------------ the arithmetics
class Bound:
    """float64 with a running bound: a value is (v, a, b), the fp32 result lies within a + P * b of v."""

    def __init__(self, flips=(), P=P_ASSERT):
        self.flips, self.P = frozenset(flips), P
        self.args, self.conds = [], []                       # per select, in call order
        self.near = {k: None for k in KINDS}                 # per kind: any of its selects near its knee, per element

    def lift(self, x):
        if isinstance(x, tuple):
            return x
        v = np.asarray(x, np.float64)
        z = np.zeros_like(v)
        return (v, z, z)

    @staticmethod
    def _rnd(z, a, b):
        return (z, a + 0.5 * U * np.abs(z) + FLOOR, b)

    def add(self, x, y):
        x, y = self.lift(x), self.lift(y)
        return self._rnd(x[0] + y[0], x[1] + y[1], x[2] + y[2])

    def sub(self, x, y):
        x, y = self.lift(x), self.lift(y)
        return self._rnd(x[0] - y[0], x[1] + y[1], x[2] + y[2])

    def mul(self, x, y):
        x, y = self.lift(x), self.lift(y)
        ax, ay = np.abs(x[0]), np.abs(y[0])
        return self._rnd(x[0] * y[0], ay * x[1] + ax * y[1], ay * x[2] + ax * y[2])

    def div(self, x, y):
        x, y = self.lift(x), self.lift(y)
        z = x[0] / y[0]
        dx, dy = 1.0 / np.abs(y[0]), np.abs(z / y[0])
        return self._rnd(z, dx * x[1] + dy * y[1], dx * x[2] + dy * y[2])

    def pow(self, x, p):
        x = self.lift(x)
        z = np.power(x[0], p)
        d = np.abs(p * np.power(x[0], p - 1.0))
        return (z, d * x[1] + FLOOR, d * x[2] + U * np.abs(z))

    def clamp(self, x, lo, hi):
        x = self.lift(x)
        e = x[1] + self.P * x[2]
        sure = (lo is not None and x[0] < lo - e) | (hi is not None and x[0] > hi + e)       # the fp32 value is clamped too
        keep = np.where(sure, 0.0, 1.0)
        return (np.clip(x[0], lo, hi), x[1] * keep, x[2] * keep)

    def select(self, kind, x, thr, hi_fn, lo_fn, safe):
        x = self.lift(x)
        e = x[1] + self.P * x[2]
        cond = x[0] > thr
        near = (np.abs(x[0] - thr) <= e) & (e > 0)           # an exact argument takes the kernel's branch, on the knee too
        self.args.append(x[0])
        self.conds.append(cond)
        self.near[kind] = near if self.near[kind] is None else (self.near[kind] | near)
        take = cond ^ near if kind in self.flips else cond
        xh = tuple(np.where(take, x[0], safe) if i == 0 else np.where(take, x[i], 0.0) for i in range(3))
        hi, lo = self.lift(hi_fn(xh)), self.lift(lo_fn(x))
        return tuple(np.where(take, h, l) for h, l in zip(hi, lo))


class Plain:
    """the same operations in one dtype, rounding as the dtype rounds; `forced` replays another run's select decisions"""

    def __init__(self, dtype, forced=None, pow_off=0.0):
        self.dtype, self.forced, self.pow_off = dtype, forced, pow_off       # pow_off: a pow that is off by that many U * |z|
        self.args, self.conds = [], []

    def lift(self, x):
        return np.asarray(x, self.dtype)

    def add(self, x, y):
        return self.lift(x) + self.lift(y)

    def sub(self, x, y):
        return self.lift(x) - self.lift(y)

    def mul(self, x, y):
        return self.lift(x) * self.lift(y)

    def div(self, x, y):
        return self.lift(x) / self.lift(y)

    def pow(self, x, p):
        z = np.power(self.lift(x), self.lift(p))
        return z * self.lift(1.0 + self.pow_off * U) if self.pow_off else z

    def clamp(self, x, lo, hi):
        # fminf(fmaxf(v, lo), hi) on finite values
        x = self.lift(x)
        if lo is not None:
            x = np.maximum(x, self.lift(lo))
        if hi is not None:
            x = np.minimum(x, self.lift(hi))
        return x

    def select(self, kind, x, thr, hi_fn, lo_fn, safe):
        x = self.lift(x)
        cond = x > self.lift(thr) if self.forced is None else self.forced[len(self.conds)]
        self.args.append(x)
        self.conds.append(cond)
        hi, lo = hi_fn(np.where(cond, x, self.lift(safe))), lo_fn(x)
        return np.where(cond, hi, lo)


# ------------------------------------------------------------------------------------------------ luminance_px, once
def constants(fault=None):
    """K, or K with the one constant a planted fault replaces (test_color_host.py)"""
    k = dict(K, xyz=[list(r) for r in K["xyz"]], rgb=[list(r) for r in K["rgb"]])
    if fault == "g_y":
        k["rgb"][1][1] = c32(1.876)                          # 1.87599 -> 1.876
    elif fault == "zn_inv":
        k["zn_inv"] = c32(1.0888)                            # 1.08883 -> 1.0888 where Z is rebuilt
    elif fault == "zn":
        k["zn"] = c32(1.0888)                                # ... where the stylised z is normalised
    elif fault == "finv_m":
        k["finv_m"] = c32(7.78)                              # 7.787 -> 7.78 in lab_finv
    elif fault == "gamma":
        k["gamma"] = c32(2.3999)
    elif fault == "y_b":
        k["xyz"][1][2] = c32(0.07217)                        # 0.072169 -> 0.07217
    return k


def _srgb_to_linear(ar, v, k):
    return ar.select("srgb", v, k["srgb_knee"], lambda x: ar.pow(ar.div(ar.add(x, k["srgb_a"]), k["srgb_d"]), k["gamma"]),
                     lambda x: ar.div(x, k["srgb_lin"]), 0.5)


def _lab_f(ar, t, k):
    return ar.select("lab_f", t, k["lab_knee"], lambda x: ar.pow(x, k["third"]),
                     lambda x: ar.add(ar.mul(k["lab_m"], x), k["lab_o"]), 0.5)


def _lab_finv(ar, f, k):
    return ar.select("lab_finv", f, k["finv_knee"], lambda x: ar.mul(ar.mul(x, x), x),
                     lambda x: ar.div(ar.sub(x, k["lab_o"]), k["finv_m"]), 0.5)


def _linear_to_srgb(ar, v, k):
    v = ar.clamp(v, 0.0, None)
    return ar.select("out", v, k["out_knee"], lambda x: ar.sub(ar.mul(k["out_m"], ar.pow(x, k["inv_gamma"])), k["out_a"]),
                     lambda x: ar.mul(k["out_lin"], x), 0.5)


def _row(ar, m, p, q, r):
    return ar.add(ar.add(ar.mul(m[0], p), ar.mul(m[1], q)), ar.mul(m[2], r))


def luminance(ar, c, s, fault=None):
    """luminance_px in the arithmetic `ar`: c, s = three channel arrays each (content in [0,1], stylised anything finite) ->
    three output channels.  Select call order: content sRGB x3, content lab_f(y), stylised sRGB x3, lab_f x / y / z,
    lab_finv xi / yi / zi, sRGB encode r / g / b."""
    k = constants(fault)
    cl = [_srgb_to_linear(ar, v, k) for v in c]
    L_rs = ar.clamp(ar.div(ar.sub(ar.sub(ar.mul(116.0, _lab_f(ar, _row(ar, k["xyz"][1], *cl), k)), 16.0), 50.0), 50.0), -1.0, 1.0)
    if fault != "no_sty_clamp":
        s = [ar.clamp(v, 0.0, 1.0) for v in s]
    sl = [_srgb_to_linear(ar, v, k) for v in s]
    x, y, z = (_row(ar, k["xyz"][i], *sl) for i in range(3))
    fx, fy, fz = _lab_f(ar, ar.div(x, k["xn"]), k), _lab_f(ar, y, k), _lab_f(ar, ar.div(z, k["zn"]), k)
    a_rs = ar.clamp(ar.div(ar.mul(500.0, ar.sub(fx, fy)), 110.0), -1.0, 1.0)
    b_rs = ar.clamp(ar.div(ar.mul(200.0, ar.sub(fy, fz)), 110.0), -1.0, 1.0)
    if fault == "L_from_stylised":
        L_rs = ar.clamp(ar.div(ar.sub(ar.sub(ar.mul(116.0, fy), 16.0), 50.0), 50.0), -1.0, 1.0)
    if fault == "swap_ab":
        a_rs, b_rs = b_rs, a_rs
    L, a, b = ar.add(ar.mul(L_rs, 50.0), 50.0), ar.mul(a_rs, 110.0), ar.mul(b_rs, 110.0)
    yi = ar.div(ar.add(L, 16.0), 116.0)
    xi = ar.add(ar.div(a, 500.0), yi)
    zi = ar.sub(yi, ar.div(b, 200.0))
    if fault != "no_zi_max":
        zi = ar.clamp(zi, 0.0, None)
    X, Y, Z = ar.mul(_lab_finv(ar, xi, k), k["xn_inv"]), _lab_finv(ar, yi, k), ar.mul(_lab_finv(ar, zi, k), k["zn_inv"])
    return [ar.clamp(_linear_to_srgb(ar, _row(ar, k["rgb"][i], X, Y, Z), k), 0.0, 1.0) for i in range(3)]


CALLS = {"srgb_c": (0, 1, 2), "lab_f_c": (3,), "srgb_s": (4, 5, 6), "lab_f_s": (7, 8, 9), "lab_finv": (10, 11, 12), "out": (13, 14, 15)}


# ------------------------------------------------------------------------------------------------ entry, epilogue
def content_of_bytes(u8):
    """the uint8 entry: (float)u8 / 255.f, a true (correctly rounded) float32 division"""
    return np.asarray(u8, np.uint8).astype(np.float32) / np.float32(255.0)


def _channels(a, dtype):
    a = np.asarray(a)
    assert a.ndim == 2 and a.shape[1] == 3, a.shape
    return [a[:, i].astype(dtype) for i in range(3)]


class Variant:
    """one legitimate reading of the selects: ref [N,3] float64 with the bound A + P * Bp, and the epilogue's t = 255 * ref with
    its bound tA + P * tBp"""

    def __init__(self, ar, out):
        st = lambda i: np.stack([o[i] for o in out], 1)                      # noqa: E731
        self.ref, self.A, self.Bp = st(0), st(1), st(2)
        t = [ar.mul(o, 255.0) for o in out]
        self.t, self.tA, self.tBp = (np.stack([o[i] for o in t], 1) for i in range(3))

    def bound(self, P=P_ASSERT):
        return self.A + P * self.Bp

    def take(self, idx):
        v = object.__new__(Variant)
        for k in ("ref", "A", "Bp", "t", "tA", "tBp"):
            setattr(v, k, getattr(self, k)[idx])
        return v

    def bytes_range(self, P=P_ASSERT):
        """the bytes `(uint8)clamp(t)` can be for a t within the bound: lowest, the reference's own, highest"""
        e = self.tA + P * self.tBp
        q = lambda v: np.floor(np.clip(v, 0.0, 255.0)).astype(np.int64)      # noqa: E731
        return q(self.t - e), q(self.t), q(self.t + e)


class Reference:
    def __init__(self, variants, near, conds):
        self.variants, self.near, self.conds = variants, near, conds

    @property
    def ref(self):
        return self.variants[0].ref

    def take(self, idx):
        """the reference of the pixels idx, in that order (a layout of the set on a frame)"""
        return Reference([v.take(idx) for v in self.variants], {k: n[idx] for k, n in self.near.items()}, None)


def reference(content, stylised, P=P_ASSERT):
    """content [N,3] float32 (or uint8: the byte entry), stylised [N,3] float32 -> Reference: variants[0] is as computed, the
    others flip the selects of a subset of kinds on the elements near that kind's knee; near[kind] marks those pixels."""
    if np.asarray(content).dtype == np.uint8:
        content = content_of_bytes(content)
    assert np.asarray(content).dtype == np.float32 and np.asarray(stylised).dtype == np.float32
    c, s = _channels(content, np.float64), _channels(stylised, np.float64)
    with np.errstate(all="ignore"):
        ar = Bound((), P)
        out = luminance(ar, c, s)
        near = {k: np.zeros(len(c[0]), bool) if ar.near[k] is None else ar.near[k] for k in KINDS}
        variants = [Variant(ar, out)]
        live = [k for k in KINDS if near[k].any()]
        for r in range(1, len(live) + 1):
            for flips in itertools.combinations(live, r):
                av = Bound(flips, P)
                variants.append(Variant(av, luminance(av, c, s)))
    return Reference(variants, near, ar.conds)


def twin(content, stylised, conds, dtype=np.longdouble):
    """the value path in `dtype` under the float64 run's select decisions: [N,3]"""
    if np.asarray(content).dtype == np.uint8:
        content = content_of_bytes(content)
    with np.errstate(all="ignore"):
        ar = Plain(dtype, forced=conds)
        return np.stack(luminance(ar, _channels(content, dtype), _channels(stylised, dtype)), 1)


def select_args(content, stylised):
    """the 16 select arguments of a float64 evaluation, inputs taken as they are (float64 allowed): the set builders solve on
    these"""
    with np.errstate(all="ignore"):
        ar = Plain(np.float64)
        luminance(ar, _channels(content, np.float64), _channels(stylised, np.float64))
    return ar.args


def emulate(content, stylised, fault=None, pow_off=0.0):
    """the kernel in numpy float32 (no contraction; numpy's float32 power, every result of it pushed up by pow_off * U * |z| if
    asked), with a planted fault if named: [N,3] float32 and the select decisions it took"""
    if np.asarray(content).dtype == np.uint8:
        content = content_of_bytes(content)
    with np.errstate(all="ignore"):
        ar = Plain(np.float32, pow_off=pow_off)
        out = np.stack(luminance(ar, _channels(content, np.float32), _channels(stylised, np.float32), fault), 1)
    assert out.dtype == np.float32
    return out, ar.conds


def quantise(out32, fault=None):
    """quantize_u8: * 255 in float32, clamp to [0, 255], truncate"""
    t = np.clip(np.asarray(out32, np.float32) * np.float32(255.0), np.float32(0.0), np.float32(255.0))
    return (np.rint(t) if fault == "round" else np.trunc(t)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the comparisons
def check_float(got, R, P=P_ASSERT):
    """got [N,3] float32 against every variant -> (ok [N,3] bool, worst error / bound, P_needed): an element passes if it is
    within A + P * Bp of some variant; P_needed is the smallest P at which all pass (0 if A alone suffices)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == R.ref.shape, (got.dtype, got.shape)
    g = got.astype(np.float64)
    ratio = np.full(g.shape, np.inf)
    need = np.full(g.shape, np.inf)
    with np.errstate(all="ignore"):
        for v in R.variants:
            err = np.abs(g - v.ref)
            err = np.where(np.isfinite(err), err, np.inf)
            bound = v.A + P * v.Bp
            ratio = np.minimum(ratio, np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf)))
            need = np.minimum(need, np.where(err <= v.A, 0.0, np.where(v.Bp > 0, (err - v.A) / v.Bp, np.inf)))
    return ratio <= 1.0, float(ratio.max()), float(need.max())


def check_bytes(got, R, P=P_ASSERT):
    """got [N,3] uint8 -> (ok [N,3] bool, bytes that differ from variant 0's, the largest difference): a byte passes if, for
    some variant, it is within one count of that variant's byte and is a byte the epilogue can give for a value within the
    bound: it differs only where 255 * ref is within the bound of an integer (a saturated 255 is one; a value clamped at 0
    beyond its bound is not)."""
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == R.ref.shape, (got.dtype, got.shape)
    d = got.astype(np.int64)
    ok = np.zeros(d.shape, bool)
    for v in R.variants:
        lo, mid, hi = v.bytes_range(P)
        ok |= (lo <= d) & (d <= hi) & (np.abs(d - mid) <= 1)
    mid0 = R.variants[0].bytes_range(P)[1]
    return ok, int((d != mid0).sum()), int(np.abs(d - mid0).max())


def near_integer(v, P=P_ASSERT):
    """where the unclamped 255 * ref of a variant is within its bound of an integer, and which values are unclamped"""
    e = v.tA + P * v.tBp
    free = (v.ref > 0.0) & (v.ref < 1.0)
    return (np.abs(v.t - np.rint(v.t)) <= e) & free, free


# ------------------------------------------------------------------------------------------------ the input sets
def _rng(seed):
    return np.random.default_rng(seed)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def neighbours(x, k):
    """the float32 k ulps from the positive float32 x (k < 0: towards zero)"""
    x = _f32(x)
    assert (x > 0).all()
    return (x.view(np.int32) + np.int32(k)).view(np.float32)


OFFSETS = (0, 1, -1, 2, -2, 8, -8)


def _spread(p):
    """float32 of the solved parameters and its neighbours at +-1, +-2, +-8 ulps: [len(p) * 7], and the index of each"""
    p32 = _f32(p)
    return np.concatenate([neighbours(p32, k) for k in OFFSETS]), np.tile(np.arange(len(p32)), len(OFFSETS))


def _solve(make, call, thr, lo, hi, n, iters=64):
    """per pixel, the parameter in [lo, hi] at which select argument `call` of make(p) = (content, stylised) equals thr, by
    bisection in float64; (p, valid): valid where [lo, hi] brackets the threshold and the solution reaches it"""
    f = lambda p: select_args(*make(p))[call] - thr                          # noqa: E731
    a, b = np.full(n, lo, np.float64), np.full(n, hi, np.float64)
    fa, fb = f(a), f(b)
    valid = (fa * fb < 0)
    rising = fb > fa
    for _ in range(iters):
        m = 0.5 * (a + b)
        up = (f(m) < 0) == rising
        a, b = np.where(up, m, a), np.where(up, b, m)
    p = 0.5 * (a + b)
    return p, valid & (np.abs(f(p)) <= 1e-9 * thr)


def build_uniform(mode="f32", n=16384, seed=11):
    g = _rng(seed)
    c = g.integers(0, 256, (n, 3), dtype=np.uint8) if mode == "u8" else _f32(g.random((n, 3)))
    return c, _f32(g.random((n, 3)) * 1.6 - 0.3)


def build_dark(mode="f32", n=16384, seed=12):
    g = _rng(seed)
    c = g.integers(0, 21, (n, 3), dtype=np.uint8) if mode == "u8" else _f32(g.random((n, 3)) * 0.08)
    return c, _f32(g.random((n, 3)) * 0.08)


def build_identity(mode="f32", n=8192, seed=13):
    g = _rng(seed)
    if mode == "u8":
        c = g.integers(0, 256, (n, 3), dtype=np.uint8)
        return c, content_of_bytes(c)
    c = _f32(g.random((n, 3)))
    c[: n // 4] *= np.float32(0.08)
    return c, c.copy()


def build_bytes(mode="f32", seed=14):
    """content from all 256 byte values per channel: a random 3-channel draw (every value in every channel) and the grey ramp"""
    g = _rng(seed)
    draw = np.stack([g.permutation(np.repeat(np.arange(256, dtype=np.uint8), 32)) for _ in range(3)], 1)      # 8192 pixels
    ramp = np.repeat(np.arange(256, dtype=np.uint8), 8)[:, None].repeat(3, 1)                                 # 2048 pixels
    c = np.concatenate([draw, ramp])
    s = _f32(g.random((len(c), 3)) * 1.6 - 0.3)
    return (c if mode == "u8" else content_of_bytes(c)), s


def build_gamut(mode="f32"):
    """stylised at the 26 surface points of the {0, 1/2, 1}^3 grid (8 corners, 12 edge and 6 face midpoints) and at the same
    points pushed out of range ({-0.3, 1/2, 1.3}^3: the stylised clamp), each against a content grey ramp over all 256 byte
    levels.  Against the black and the white corner a grey content comes back as itself, every 255 * ref on an integer, which
    says nothing about the clamps and blurs the byte comparison: those two get the ramp (k, k, 255 - k) instead."""
    grid = [p for p in itertools.product((0, 1, 2), repeat=3) if p != (1, 1, 1)]
    pts = np.concatenate([np.array((0.0, 0.5, 1.0), np.float32)[np.array(grid)], np.array((-0.3, 0.5, 1.3), np.float32)[np.array(grid)]])
    ramp = np.arange(256, dtype=np.uint8)
    c = np.tile(ramp, len(pts))[:, None].repeat(3, 1).reshape(len(pts), 256, 3)
    for i, p in enumerate(grid + grid):
        if p in ((0, 0, 0), (2, 2, 2)):
            c[i, :, 2] = 255 - ramp
    c = c.reshape(-1, 3)
    s = np.repeat(pts, 256, 0)
    return (c if mode == "u8" else content_of_bytes(c)), _f32(s)


def build_knees(mode="f32", m=40, seed=15):
    """Every select's argument on its threshold and on the float32 neighbours of the input that puts it there.  The sRGB decode
    takes its argument from the input itself, so that one is set directly.  The others are solved per pixel in float64 for one
    free input (a grey level or one channel, content side or stylised side), then float32 neighbours of the solution are taken.
    With byte content (`u8`) only the stylised side is free.  Returns (content, stylised, group) with a name per pixel."""
    g = _rng(seed)
    u8 = mode == "u8"
    cs, ss, names = [], [], []

    def rand_content(n, lo=0, hi=256):
        b = g.integers(lo, hi, (n, 3), dtype=np.uint8)
        return content_of_bytes(b).astype(np.float64)

    def grey_bytes(n, lo, hi):
        return content_of_bytes(g.integers(lo, hi, (n, 1), dtype=np.uint8).repeat(3, 1)).astype(np.float64)

    def emit(name, c, s):
        cs.append(_f32(c)), ss.append(_f32(s)), names.extend([name] * len(c))

    def put(base, idx, ch, vals):
        """base[idx] with channel ch (None: all three) replaced by vals"""
        a = np.array(base, np.float64)[idx]
        if ch is None:
            a[:] = np.asarray(vals, np.float64)[:, None]
        else:
            a[:, ch] = vals
        return a

    def solved(name, call, thr, lo, hi, side, ch, c0, s0):
        """solve channel `ch` (None: grey) of `side` so that select `call` sits on thr; emit the neighbours"""
        n = len(c0)
        every = np.arange(n)
        make = (lambda p: (put(c0, every, ch, p), s0)) if side == "c" else (lambda p: (c0, put(s0, every, ch, p)))
        p, valid = _solve(make, call, thr, lo, hi, n)
        p, c0v, s0v = p[valid], c0[valid], s0[valid]
        if not len(p):
            return
        vals, idx = _spread(p)
        if side == "c":
            emit(name, put(c0v, idx, ch, vals.astype(np.float64)), s0v[idx])
        else:
            emit(name, c0v[idx], put(s0v, idx, ch, vals.astype(np.float64)))

    # sRGB decode: the argument is the input.  Grey and one channel, stylised side (and content side for float content)
    thr = np.float32(K["srgb_knee"])
    direct = np.concatenate([neighbours(np.full(m // 4, thr, np.float32), k) for k in OFFSETS])
    n = len(direct)
    for side in ("s",) if u8 else ("s", "c"):
        for ch in (None, 0, 1, 2):
            c0 = rand_content(n)
            s0 = g.random((n, 3)) * 1.6 - 0.3
            every = np.arange(n)
            if side == "s":
                emit("srgb", c0, put(s0, every, ch, direct))
            else:
                emit("srgb", put(c0, every, ch, direct), s0)
    # Lab f on the stylised side: x / xn, y, z / zn; grey, and the channel that drives each most
    for call, ch in ((8, None), (7, 0), (8, 1), (9, 2), (7, None), (9, None)):
        s0 = g.random((m, 3)) * (0.12 if ch is not None else 1.0)
        solved("lab_f", call, K["lab_knee"], 1e-4, 1.0, "s", ch, rand_content(m), s0)
    # ... and on the content's y
    if not u8:
        for ch in (None, 0, 1, 2):
            c0 = g.random((m, 3)) * (0.1 if ch is not None else 1.0)
            solved("lab_f", 3, K["lab_knee"], 1e-4, 1.0, "c", ch, c0, g.random((m, 3)) * 1.6 - 0.3)
    # the inverse: yi from the content's L; xi and zi from the stylised chroma against a content whose L is near 8
    if not u8:
        for ch in (None, 1):
            c0 = g.random((m, 3)) * (0.1 if ch is not None else 1.0)
            solved("lab_finv", 11, K["finv_knee"], 1e-4, 1.0, "c", ch, c0, g.random((m, 3)))
    for call, ch in ((10, 0), (10, 1), (12, 2), (12, 1)):
        for lo_b, hi_b in ((20, 32), (10, 120)):                 # L near 8 (both of xi, yi near the knee), and well above it
            c0 = grey_bytes(m, lo_b, hi_b)
            if not u8:
                c0 = c0 + (g.random((m, 3)) - 0.5) * 0.01
            solved("lab_finv", call, K["finv_knee"], 1e-4, 1.0, "s", ch, c0, g.random((m, 3)) * 0.5)
    # sRGB encode: each output channel's linear value on 0.0031308, by a stylised channel against a dark content, and by the
    # content's grey level
    for call in (13, 14, 15):
        for ch in (call - 13, (call - 12) % 3):
            c0 = grey_bytes(m, 4, 40)
            solved("out", call, K["out_knee"], 1e-4, 1.0, "s", ch, c0, g.random((m, 3)) * 0.3)
        if not u8:
            grey = g.random((m, 1)) * 0.3
            s0 = np.clip(grey + (g.random((m, 3)) - 0.5) * 0.1, 0.0, 1.0)
            solved("out", call, K["out_knee"], 1e-4, 0.6, "c", None, np.zeros((m, 3)), s0)
    c, s = np.concatenate(cs), np.concatenate(ss)
    if u8:
        cb = np.rint(c.astype(np.float64) * 255.0).astype(np.uint8)
        assert np.array_equal(content_of_bytes(cb), c)          # every content value above came from a byte
        c = cb
    return c, s, np.array(names)


BUILDERS = {"uniform": build_uniform, "dark": build_dark, "knees": lambda mode="f32": build_knees(mode)[:2], "gamut": build_gamut,
            "bytes": build_bytes, "identity": build_identity}
_cache = {}


def case(name, mode="f32"):
    """(content, stylised, Reference) of a named set, built and referenced once per process"""
    key = (name, mode)
    if key not in _cache:
        c, s = BUILDERS[name](mode)
        _cache[key] = (c, s, reference(c, s))
        for a in (c, s):
            a.setflags(write=False)
    return _cache[key]
