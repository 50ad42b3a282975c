"""The kernels of csrc/cwct.hip one by one (vstnet_amd.cwct.ops -> the cWCT calls of include/vstnet.h) against fp64 references
computed on the CPU at test time (tests/cwct_ops_ref.py), at the shapes, pointer offsets, masks, precisions and slot counts at
which the launchers pick each of their kernel forms (tests/test_cwct_ops_host.py proves that the tables reach every form).

Bounds.  e32 is the fp32 restatement of the device arithmetic against the fp64 reference, at the same inputs under the same
normalised metric (covariance against sqrt(C_ii C_jj), mean against sqrt(C_ii), apply against sum |T||x| + |t0|, factor against
|mixL||Lc^-1|); the device must stay within FACTOR x max(e32, floor).  FACTOR = 4 and floor = u for every op, fixed on the host
(cwct_ops_ref.py says why; the host test shows every mutant of the restatements over 1.25 x FACTOR).  The split forms are held to
the emulated split.  Exact assertions are bitwise: label counts, the constant channel, sentinel pixels and records, NaN margins,
in place against out of place, prefactored against unfactored, retry counts, plans.  Every test prints its ratio (-s) before it
asserts; DESIGN.md section 5 ("The cWCT kernels one by one") has the table of measured ratios.

Measured on an MI355X (x max(e32, floor), bound 4; 531 cases): statistics unmasked at most 1.61 (N = 16), 1.51 (MFMA, VEC or
not), 2.27 at L = 2^21 + 68 (the capped groups; 2.17 with 2048-pixel groups, 1.26 with 1024), one label 1.35, plan form 2.35
(N = 64, 32 slots, 8 passes), packed rows 0.81 / 1.32 (rectangle) for rows of 32 and 0.47 / 1.26 for rows of 128, packed labels
1.41; factor 1.16, with jitter 1.37, from a minimum retry count 1.35; apply 2.22 (scalar FMA), 1.25 (vector FMA), 1.00 (fp32
MFMA, every width), split 1.01 of the emulated split (itself at most 1.45e-5 of the claimed 1.5e-5); apply_labels 1.00 (fp32)
and 1.01 (split); packed apply 1.51 / 1.15, packed labels 1.15.

Three cases found something, before the fixes that are now in csrc/cwct.hip:
  * test_factor[128-*]: the affine of a prefactored style record was not the unfactored one's bits at N = 128 (rows 48 and up of T,
    one ulp).  The compiler had fused every `r -= li * lk` of the Cholesky into an fma in cwct_prefactor_kernel<8> and all but one
    packed pair in cwct_factor_kernel<8>; the update is now an explicit fma.
  * test_stats[16-1729-0-scales] (6.96 x), [16-516-*] (5.11), [16-192-*] (4.57), [16-1729-0-outlier] (4.30): the N = 16 kernel
    summed a workgroup's 512 pixels in one fmaf chain per entry; it now sums each 64-pixel tile apart.
  * test_stats[128-516-*] (4.09 x) and [128-1729-0-outlier] (4.01): the same in the MFMA kernel at N = 128, where one wave owns all
    64 pixels of every tile (256 dependent accumulations); the tile's MFMAs now have accumulators of their own.
test_factor_jitter[32-indefinite] sat at 7.15 x while the restatement's Cholesky update was a product and a subtraction: the device
fuses them, and at that conditioning the two evaluations are 7.1 x apart on the host as well; the restatement now restates the fma."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cwct_ops_ref as O                                               # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 256                     # floats (bytes of a mask) on either side of a guarded view: keeps the view's own alignment


@pytest.fixture(scope="module")
def ops():
    from vstnet_amd.cwct import ops
    return ops


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """a HIP error is sticky: nothing more is started on the card once a call has failed"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                            # noqa: BLE001
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else (np.uint64 if a.dtype == np.float64 else np.uint8))


class Guarded:
    """An [N, L] fp32 array at element offset `off` from a 256-byte boundary, inside a buffer whose margins hold NaN"""

    def __init__(self, shape, off=0, fill=None, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.a = PAD + off
        nan = float("nan") if dtype.is_floating_point else 0xEE
        self.buf = torch.full((self.a + self.n + PAD,), nan, dtype=dtype, device="cuda")
        self.view = self.buf[self.a:self.a + self.n].view(*shape)
        assert (self.view.data_ptr() - self.buf.data_ptr()) == self.a * self.buf.element_size() and self.buf.data_ptr() % 256 == 0
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill)))
        self.margins = (self.buf[:self.a].clone(), self.buf[self.a + self.n:].clone())

    def check(self):
        torch.cuda.synchronize()
        lo, hi = self.buf[:self.a], self.buf[self.a + self.n:]
        assert bits(lo.cpu().numpy()).tobytes() == bits(self.margins[0].cpu().numpy()).tobytes(), "margin written"
        assert bits(hi.cpu().numpy()).tobytes() == bits(self.margins[1].cpu().numpy()).tobytes(), "margin written"
        return self.view.cpu().numpy()


def at_offset(a, off, dtype=torch.float32):
    return Guarded(a.shape, off, fill=a, dtype=dtype).view


def exact_constant_channel(got, N):
    _, m, c = O.unpack(got, N)
    assert m[O.CONST_CH] == O.CONST_VAL and not c[O.CONST_CH].any() and not c[:, O.CONST_CH].any(), "constant channel"


# -------------------------------------------------------------------------------------------------------- statistics
_STATS = {}


def stats_refs(N, L, kind):
    """input, fp64 reference and restatement of an unmasked case, shared by its offsets"""
    key = (N, L, kind)
    if key not in _STATS:
        x = O.stats_input(N, L, kind)
        _STATS[key] = (x, O.stats64(x), O.stats32(x))
    return _STATS[key]


@pytest.mark.parametrize("N,L,off,kind", O.STATS_CASES, ids=lambda v: str(v))
def test_stats(ops, N, L, off, kind):
    x, want, r32 = stats_refs(N, L, kind)
    rec = Guarded((O.rec_len(N),), 0, dtype=torch.float64)
    ops.stats(at_offset(x, off), out=rec.view)
    got = rec.check()
    r, (gc, gm, ec, em) = O.stats_ratio(got, r32, want, N, skip=(O.CONST_CH,))
    print(f"stats N={N} L={L} off={off} {kind} [{O.stats_form(N, L, off)}]: e32 cov {ec / O.U:.3g} u mean {em / O.U:.3g} u, "
          f"device cov {gc / O.U:.3g} u mean {gm / O.U:.3g} u = {r:.2f} x max(e32, floor), bound {O.FACTOR['stats']}")
    assert got[0] == L
    exact_constant_channel(got, N)
    assert r <= O.FACTOR["stats"], (N, L, off, kind, r)


@pytest.mark.parametrize("L", O.STATS_LONG)
def test_stats_long(ops, L):
    x = O.long_input(L)
    want, r32 = O.stats64_chunked(x), O.stats32(x)
    got = ops.stats(dev(x)).cpu().numpy()
    r, (gc, gm, ec, em) = O.stats_ratio(got, r32, want, 32, skip=(O.CONST_CH,))
    print(f"stats N=32 L={L} [{O.stats_groups(L)}]: e32 cov {ec / O.U:.3g} u mean {em / O.U:.3g} u, device cov {gc / O.U:.3g} u "
          f"mean {gm / O.U:.3g} u = {r:.2f} x max(e32, floor), bound {O.FACTOR['stats']}")
    assert got[0] == L
    exact_constant_channel(got, 32)
    assert r <= O.FACTOR["stats"], (L, r)


@pytest.mark.parametrize("N,L,moff,label", O.MASK_CASES, ids=lambda v: str(v))
def test_stats_one_label(ops, N, L, moff, label):
    x, mask = O.stats_input(N, L, "scales", seed=1), O.one_label_mask(L)
    sel = mask == label
    want, r32 = O.stats64(x, sel), O.stats32(x, mask, label)
    got = ops.stats(dev(x), mask=at_offset(mask, moff, torch.uint8), label=label).cpu().numpy()
    r, (gc, gm, ec, em) = O.stats_ratio(got, r32, want, N, skip=(O.CONST_CH,))
    print(f"stats N={N} L={L} label={label} ({int(sel.sum())} px) mask+{moff} [{O.stats_form(N, L, 0, moff)}]: e32 cov {ec / O.U:.3g} u, "
          f"device cov {gc / O.U:.3g} u mean {gm / O.U:.3g} u = {r:.2f} x, bound {O.FACTOR['stats']}")
    assert got[0] == sel.sum()                                        # the count is exact
    exact_constant_channel(got, N)
    assert r <= O.FACTOR["stats"], (N, L, moff, label, r)


def device_plan(ops, cm, sm):
    plan = ops.label_plan(dev(cm), dev(sm))
    n, over, lut, slot_label = ops.plan_info(plan)
    rl, labels, rover = O.plan_ref(cm, sm)
    assert n == len(labels) and over == rover and (lut == rl).all() and slot_label[:n].tolist() == labels, "plan"
    return plan, rl, n


def slot_ratios(got, r32, want, n, N):
    worst = 0.0
    for s in range(n):
        assert got[s, 0] == want[s, 0], ("count", s)
        exact_constant_channel(got[s], N)
        worst = max(worst, O.stats_ratio(got[s], r32[s], want[s], N, skip=(O.CONST_CH,))[0])
    assert bits(got[n:]).tobytes() == bits(np.full_like(got[n:], O.SENTINEL_F64)).tobytes(), "records past n_slots written"
    return worst


@pytest.mark.parametrize("N,L,n,max_slots,kind", O.PLAN_CASES, ids=lambda v: str(v))
def test_stats_labels(ops, N, L, n, max_slots, kind):
    x = O.plan_input(N, L)
    cm, sm = O.plan_mask(L, n, kind, N)
    plan, lut, n_dev = device_plan(ops, cm, sm)
    assert n_dev == n
    want, r32 = O.stats_labels64(x, cm, lut, n), O.stats_labels32(x, cm, lut, n, max_slots)
    out = torch.full((O.MAX_SLOTS, O.rec_len(N)), O.SENTINEL_F64, dtype=torch.float64, device="cuda")
    ops.stats_labels(dev(x), dev(cm), plan, max_slots, out=out)
    r = slot_ratios(out.cpu().numpy(), r32, want, n, N)
    print(f"stats_labels N={N} L={L} slots={n} max_slots={max_slots} {kind} [{O.stats_labels_passes(N, max_slots)} passes]: "
          f"device {r:.2f} x max(e32, floor), bound {O.FACTOR['stats']}")
    assert r <= O.FACTOR["stats"], (N, L, n, max_slots, kind, r)


# ------------------------------------------------------------------------------------------------------- packed rows
def packed(ops, sp, H, W):
    """z, its packed code on the device and the code's rows on the host; every row is the channel vector of the pixel the
    restated row order gives (as a multiset: the order of the channels within a row is the code's own)"""
    z = O.code_input(sp, H, W)
    code = ops.z_to_code(dev(z), H, W, sp)
    N = z.shape[0]
    rows = code.cpu().numpy().reshape(-1, N)
    y, x = O.row_pixels(H, W, sp)
    assert (np.sort(rows, axis=1) == np.sort(z[:, y, x].T, axis=1)).all(), "row order"
    return code, rows, N


@pytest.mark.parametrize("sp,H,W,rect", O.CODE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_stats_code(ops, sp, H, W, rect):
    code, rows, N = packed(ops, sp, H, W)
    const = int(np.nonzero((rows == O.CONST_VAL).all(0))[0][0])
    inside = O.rect_rows(H, W, sp, rect)
    L, per = O.code_groups(H, W, sp)
    want = O.stats64(rows.T, inside)
    r32 = O.stats32(np.ascontiguousarray(rows.T), inside.astype(np.uint8), 1, groups=(-(-L // per), per, "code"))
    rec = Guarded((O.rec_len(N),), 0, dtype=torch.float64)
    if rect is None:
        ops.stats_code(code, H, W, sp, out=rec.view)
    else:
        ops.stats_code_rect(code, H, W, sp, rect, out=rec.view)
    got = rec.check()
    r, (gc, gm, ec, em) = O.stats_ratio(got, r32, want, N, skip=(const,))
    print(f"stats_code sp={sp} {H}x{W} rect={rect} [{O.stats_code_form(H, W, sp, rect)}]: e32 cov {ec / O.U:.3g} u, device cov "
          f"{gc / O.U:.3g} u mean {gm / O.U:.3g} u = {r:.2f} x, bound {O.FACTOR['stats']}")
    _, m, c = O.unpack(got, N)
    assert got[0] == inside.sum() and m[const] == O.CONST_VAL and not c[const].any() and not c[:, const].any()
    assert r <= O.FACTOR["stats"], (sp, H, W, rect, r)
    if rect is None:                                                  # the full rectangle runs exactly the plain call
        assert bits(ops.stats_code_rect(code, H, W, sp, (0, 0, H, W)).cpu().numpy()).tobytes() == bits(got).tobytes()


@pytest.mark.parametrize("H,W,n,rect", O.CODE_LABEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_stats_labels_code(ops, H, W, n, rect):
    code, rows, N = packed(ops, 2, H, W)
    mask = O.code_label_mask(H, W, n)
    plan, lut, n_dev = device_plan(ops, mask, mask)
    assert n_dev == n
    mrows = ops.mask_to_code(dev(mask), H, W)
    y, x = O.row_pixels(H, W, 2)
    assert (mrows.cpu().numpy() == mask[y, x]).all()
    inside = O.rect_rows(H, W, 2, rect)
    slotless = int(np.nonzero(lut == 255)[0][0])
    meff = np.where(inside, mask[y, x], slotless).astype(np.uint8)
    L, per = O.labels_code_groups(H, W)
    xt = np.ascontiguousarray(rows.T)
    want = O.stats_labels64(xt, meff, lut, n)
    r32 = O.stats_labels32(xt, meff, lut, n, n, groups=(-(-L // per), per, "code"))
    out = torch.full((O.MAX_SLOTS, O.rec_len(N)), O.SENTINEL_F64, dtype=torch.float64, device="cuda")
    if rect is None:
        ops.stats_labels_code(code, H, W, mrows, plan, n, out=out)
    else:
        ops.stats_labels_code_rect(code, H, W, rect, mrows, plan, n, out=out)
    got = out.cpu().numpy()
    const = int(np.nonzero((rows == O.CONST_VAL).all(0))[0][0])
    worst = 0.0
    for s in range(n):
        assert got[s, 0] == want[s, 0], ("count", s)
        worst = max(worst, O.stats_ratio(got[s], r32[s], want[s], N, skip=(const,))[0])
    print(f"stats_labels_code {H}x{W} slots={n} rect={rect}: device {worst:.2f} x max(e32, floor), bound {O.FACTOR['stats']}")
    assert bits(got[n:]).tobytes() == bits(np.full_like(got[n:], O.SENTINEL_F64)).tobytes()
    assert worst <= O.FACTOR["stats"], (H, W, n, rect, worst)


APPLY_CODE_SHAPES = sorted({(sp, H, W) for sp, H, W, _ in O.CODE_CASES}) + [(2, 12, 20), (1, 24, 20)]     # + a partial last tile


@pytest.mark.parametrize("sp,H,W", APPLY_CODE_SHAPES, ids=lambda v: str(v))
def test_apply_code(ops, sp, H, W):
    code, rows, N = packed(ops, sp, H, W)
    aff = O.apply_input(N, 4, seed=9)[1]
    xt = np.ascontiguousarray(rows.T)
    want, den = O.apply64(xt, aff, N)
    e32 = O.apply_err(O.apply32(xt, aff, N), want, den)
    g = Guarded((rows.size,), 0)
    ops.apply_code(code, H, W, sp, dev(aff), out=g.view)
    got = g.check()
    r = O.ratio("apply", O.apply_err(got.reshape(-1, N).T, want, den), e32)
    print(f"apply_code sp={sp} {H}x{W}: e32 {e32 / O.U:.3g} u, device {r:.2f} x max(e32, floor), bound {O.FACTOR['apply']}")
    assert r <= O.FACTOR["apply"], (sp, H, W, r)
    inplace = Guarded((rows.size,), 0, fill=rows.reshape(-1))
    ops.apply_code(inplace.view, H, W, sp, dev(aff), out=inplace.view)
    assert bits(inplace.check()).tobytes() == bits(got).tobytes(), "in place"


def test_apply_labels_code(ops):
    H, W, n = 24, 40, 3
    code, rows, N = packed(ops, 2, H, W)
    mask = O.code_label_mask(H, W, n)
    plan, lut, _ = device_plan(ops, mask, mask)
    mrows = ops.mask_to_code(dev(mask), H, W)
    aff = O.affines_input(N, n)
    xt, mr = np.ascontiguousarray(rows.T), mrows.cpu().numpy()
    O.KAPP[N] = 8
    want, den = O.apply_labels_ref(xt, aff, mr, lut, n, N, O.apply64)
    r32 = O.apply_labels_ref(xt, aff, mr, lut, n, N, O.apply32)
    e32 = O.apply_err(r32, want, den)
    g = Guarded((rows.size,), 0)
    ops.apply_labels_code(code, H, W, dev(aff), mrows, plan, n, out=g.view)
    got = g.check().reshape(-1, N).T
    r = O.ratio("apply", O.apply_err(got, want, den), e32)
    print(f"apply_labels_code {H}x{W} slots={n}: e32 {e32 / O.U:.3g} u, device {r:.2f} x, bound {O.FACTOR['apply']}")
    none = lut[mr] == 255
    assert none.sum() == 6 and bits(got[:, none]).tobytes() == bits(xt[:, none]).tobytes()      # rows without a slot keep x
    assert r <= O.FACTOR["apply"]
    from vstnet_amd._lib import VstError
    with pytest.raises(VstError):
        ops.apply_labels_code(code, H, W, dev(aff), mrows, plan, 9)


# ------------------------------------------------------------------------------------------------------------ factor
def run_factor(ops, content, styles, al, ac, N, min_tries=None):
    aff, info = ops.factor(dev(content), [dev(s) for s in styles], al, N, alpha_c=ac, eps=O.EPS, min_tries=min_tries)
    return aff.cpu().numpy(), info.cpu().tolist()


@pytest.mark.parametrize("N,k,ac,cond", O.FACTOR_CASES, ids=lambda v: str(v))
def test_factor(ops, N, k, ac, cond):
    content, styles, al = O.factor_input(N, k, cond)
    a32, info32 = O.factor32(content, styles, al, ac, N)
    ref = O.factor64(content, styles, al, ac, N, info32)
    e32 = O.factor_err(a32, ref, N)
    got, info = run_factor(ops, content, styles, al, ac, N)
    r = O.ratio("factor", O.factor_err(got, ref, N), e32)
    print(f"factor N={N} styles={k} alpha_c={ac} cond={cond:g}: e32 {e32 / O.U:.3g} u, device {r:.2f} x max(e32, floor), "
          f"bound {O.FACTOR['factor']}")
    assert info == info32                                             # retry counts (none here)
    assert r <= O.FACTOR["factor"], (N, k, ac, cond, r)
    # a prefactored style record gives the same affine bit for bit
    pre, pinfo = ops.prefactor(dev(styles[0]), N, O.EPS)
    assert pinfo.cpu().tolist() == [0] and float(pre[0]) == -(styles[0][0] + 1.0)
    got2, info2 = run_factor(ops, content, [pre.cpu().numpy()] + styles[1:], al, ac, N)
    assert bits(got2).tobytes() == bits(got).tobytes() and info2 == info, "prefactored"


@pytest.mark.parametrize("kind", O.JITTER_KINDS)
@pytest.mark.parametrize("N", O.STATS_N)
def test_factor_jitter(ops, N, kind):
    content = O.jitter_content(N, kind)
    _, styles, al = O.factor_input(N, 2, 10.0)
    a32, info32 = O.factor32(content, styles, al, 0.3, N)
    ref = O.factor64(content, styles, al, 0.3, N, info32)
    e32 = O.factor_err(a32, ref, N)
    got, info = run_factor(ops, content, styles, al, 0.3, N)
    r = O.ratio("factor", O.factor_err(got, ref, N), e32)
    print(f"factor N={N} {kind}: tries {info} (restatement {info32}), e32 {e32 / O.U:.3g} u, device {r:.2f} x, bound {O.FACTOR['factor']}")
    assert info == info32, "retry counts"
    assert r <= O.FACTOR["factor"], (N, kind, r)
    # the minimum-tries entry of info: the count itself changes nothing; more is kept, for the content and for a style
    same, info_s = run_factor(ops, content, styles, al, 0.3, N, min_tries=[info[0], 0, 0, 0])
    assert info_s == info and bits(same).tobytes() == bits(got).tobytes()
    mt = [info[0] + 2, 0, 1, 0]
    more, info_m = run_factor(ops, content, styles, al, 0.3, N, min_tries=mt)
    a32m, info32m = O.factor32(content, styles, al, 0.3, N, min_tries=mt)
    assert info_m == info32m == mt
    refm = O.factor64(content, styles, al, 0.3, N, mt)
    rm = O.ratio("factor", O.factor_err(more, refm, N), O.factor_err(a32m, refm, N))
    print(f"    min_tries {mt}: device {rm:.2f} x")
    assert rm <= O.FACTOR["factor"]
    pre, pinfo = ops.prefactor(dev(content), N, O.EPS)                # the prefactor's retries are the factor's
    assert pinfo.cpu().tolist() == [info[0]]


@pytest.mark.parametrize("N", (32, 64, 128))
def test_factor_labels(ops, N):
    n, L = 5, 1092
    cm, sm = O.plan_mask(L, n, "round_robin", N)
    plan, lut, _ = device_plan(ops, cm, sm)
    labels = O.plan_labels(n)

    def block(seed, count):
        b = np.full((O.MAX_SLOTS, O.rec_len(N)), O.SENTINEL_F64)
        for s in range(count):
            b[s] = O.record(N, O.spd(N, 30.0, seed + s, scale=1.0 + 0.1 * s), seed + s)
        return b
    content, style, style2 = block(100, n), block(200, n), block(300, n)

    def single(s, srecs, al, ac):
        return run_factor(ops, content[s], srecs, al, ac, N)[0]
    sent = lambda: torch.from_numpy(np.full((O.MAX_SLOTS, N * N + N), O.SENTINEL_F32, dtype=np.float32)).cuda()    # noqa: E731
    sbits = bits(np.full((O.MAX_SLOTS - n, N * N + N), O.SENTINEL_F32, dtype=np.float32)).tobytes()

    for max_slots in (0, 8):                                          # plain: slot s = the single-pair factor of (content s, style s)
        aff, info = ops.factor_labels(dev(content), dev(style), plan, N, O.EPS, max_slots, affines=sent())
        aff, info = aff.cpu().numpy(), info.cpu().numpy()
        for s in range(n):
            assert bits(aff[s]).tobytes() == bits(single(s, [style[s]], [1.0], 0.0)).tobytes(), ("plain", s)
        assert bits(aff[n:]).tobytes() == sbits and not info.any(), "affines past n_slots written"

    # keyed: the style's records in the order of its own plan, which lacks the label of content slot 2
    lost = labels[2]
    sm2 = sm[sm != lost]
    splan, slut, sn = device_plan(ops, sm2, sm2)
    assert sn == n - 1 and slut[lost] == 255
    keyed = np.full_like(style, O.SENTINEL_F64)
    for s, lab in enumerate(labels):
        if lab != lost:
            keyed[slut[lab]] = style[s]
    aff, info = ops.factor_labels(dev(content), dev(keyed), plan, N, O.EPS, 0, style_plan=splan, affines=sent())
    aff, info = aff.cpu().numpy(), info.cpu().numpy()
    ident = np.concatenate([np.eye(N, dtype=np.float32).reshape(-1), np.zeros(N, dtype=np.float32)])
    for s in range(n):
        if s == 2:
            assert bits(aff[s]).tobytes() == bits(ident).tobytes() and info[s, 1] == 2
        else:
            assert bits(aff[s]).tobytes() == bits(single(s, [style[s]], [1.0], 0.0)).tobytes() and info[s, 1] == 0, ("keyed", s)
    assert bits(aff[n:]).tobytes() == sbits

    al = [0.25, 0.75]                                                 # mix: two styles and alpha_c, one of them keyed
    aff, info = ops.factor_labels_mix(dev(content), [dev(style2), dev(keyed)], al, plan, N, 0.3, O.EPS, n,
                                      style_plans=[None, splan], affines=sent())
    aff, info = aff.cpu().numpy(), info.cpu().numpy()
    for s in range(n):
        if s == 2:
            assert bits(aff[s]).tobytes() == bits(ident).tobytes() and info[s, 1] == 2
        else:
            assert bits(aff[s]).tobytes() == bits(single(s, [style2[s], style[s]], al, 0.3)).tobytes(), ("mix", s)
    assert bits(aff[n:]).tobytes() == sbits and info.shape == (O.MAX_SLOTS, 4)


# ------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("N,L,prec,masked", O.APPLY_CASES, ids=lambda v: str(v))
def test_apply(ops, N, L, prec, masked):
    x, aff = O.apply_input(N, L)
    mask = O.apply_mask(L) if masked else None
    on = np.ones(L, dtype=bool) if mask is None else mask == O.APPLY_LABEL
    want, den = O.apply64(x, aff, N)
    e32 = {"apply": O.apply_err(O.apply32(x, aff, N)[:, on], want[:, on], den[:, on]),
           "apply_split": O.apply_err(O.apply_split32(x, aff, N)[:, on], want[:, on], den[:, on])}
    daff, dmask = dev(aff), (None if mask is None else dev(mask))
    sent = np.full((N, L), O.SENTINEL_F32, dtype=np.float32)
    worst = {}
    for off in O.APPLY_OFFS:
        form = O.apply_form(N, L, off, off, masked, prec)
        op = "apply_split" if form == "split" else "apply"
        g = Guarded((N, L), off, fill=sent)
        ops.apply(at_offset(x, off), daff, out=g.view, mask=dmask, label=O.APPLY_LABEL, precision=prec)
        got = g.check()
        r = O.ratio(op, O.apply_err(got[:, on], want[:, on], den[:, on]), e32[op])
        worst[form] = max(worst.get(form, 0.0), r)
        assert bits(got[:, ~on]).tobytes() == bits(sent[:, ~on]).tobytes(), "pixels of another label written"
        if form != "split":
            assert (got[:, O.ZERO_PIXEL] == aff[N * N:]).all() and (got[O.ZERO_ROW, on] == aff[N * N + O.ZERO_ROW]).all()
        gi = Guarded((N, L), off, fill=x)                             # in place: the same bits, other labels keep x
        ops.apply(gi.view, daff, out=gi.view, mask=dmask, label=O.APPLY_LABEL, precision=prec)
        goti = gi.check()
        assert bits(goti[:, on]).tobytes() == bits(got[:, on]).tobytes(), ("in place", off)
        assert bits(goti[:, ~on]).tobytes() == bits(x[:, ~on]).tobytes(), ("in place, other labels", off)
        assert r <= O.FACTOR[op], (N, L, prec, masked, off, form, r)
    print(f"apply N={N} L={L} {prec} masked={masked}: e32 {e32['apply'] / O.U:.3g} u (split {e32['apply_split']:.3g}), device x max(e32, floor) "
          f"per form {({k: round(v, 2) for k, v in worst.items()})}, bound {O.FACTOR['apply']}")


@pytest.mark.parametrize("N,L,prec,n,max_slots,kind", O.APPLY_LABELS_CASES, ids=lambda v: str(v))
def test_apply_labels(ops, N, L, prec, n, max_slots, kind):
    x = O.apply_input(N, L, seed=5)[0]
    cm, sm = O.plan_mask(L, n, kind, N)
    plan, lut, _ = device_plan(ops, cm, sm)
    aff = O.affines_input(N, n)
    want, den = O.apply_labels_ref(x, aff, cm, lut, n, N, O.apply64, max_slots)
    e32 = {"apply": O.apply_err(O.apply_labels_ref(x, aff, cm, lut, n, N, O.apply32, max_slots), want, den),
           "apply_split": O.apply_err(O.apply_labels_ref(x, aff, cm, lut, n, N, O.apply_split32, max_slots), want, den)}
    none = lut[cm] == 255
    daff, dmask = dev(aff), dev(cm)
    worst = {}
    for off in (0, 1, 2):
        form, passes = O.apply_labels_form(N, L, off, off, 0, prec, max_slots)
        op = "apply_split" if form == "split" else "apply"
        g = Guarded((N, L), off)
        ops.apply_labels(at_offset(x, off), daff, dmask, plan, max_slots, prec, out=g.view)
        got = g.check()
        r = O.ratio(op, O.apply_err(got, want, den), e32[op])
        worst[form] = max(worst.get(form, 0.0), r)
        assert bits(got[:, none]).tobytes() == bits(x[:, none]).tobytes(), "pixels without a slot"
        gi = Guarded((N, L), off, fill=x)
        ops.apply_labels(gi.view, daff, dmask, plan, max_slots, prec, out=gi.view)
        assert bits(gi.check()).tobytes() == bits(got).tobytes(), ("in place", off)
        assert r <= O.FACTOR[op], (N, L, prec, n, max_slots, kind, off, form, r)
    print(f"apply_labels N={N} L={L} {prec} slots={n} max_slots={max_slots} {kind}: device x max(e32, floor) per form "
          f"{({k: round(v, 2) for k, v in worst.items()})}, bound {O.FACTOR['apply']}")
