"""The workspace contract of include/vstnet.h, family by family, through the C ABI: "outputs and workspaces are caller-provided
(vst_*_workspace_bytes tell sizes)".  Every call below gets a workspace of EXACTLY the bytes its size function states, at exactly
the alignment the header promises to accept and no better (tests/ws_guard.py: Arena), between two 64 KiB pads, and runs

    once under each fill 0xFF / 0x7F / 0x00 (NaN or -1; a huge finite number; zero),
    once more in the 0x7F arena as its own last run left it,
    and, where the header lets one workspace serve several calls of a family, again after each sibling call has run in it.

Asserted per case:
    (a) every pad of every arena and of every output buffer still holds its fill, byte for byte;
    (b) the outputs of all runs are equal bit for bit;
    (c) the 0xFF run's outputs pass the family's own check against its own reference (imported from the family's GPU test and
        *_ref module: no tolerance is new here) - so that (b) is not met by equal wrong answers;
    (d) the bytes touched lie inside [0, bytes);
    (e) the inputs are unchanged.
Printed per case (-s), and recorded in DESIGN.md ("The workspace contract"): bytes, the touched range, the unused tail.

Entry points that take `workspace_bytes` are also called with one byte less and with an address off the stated grid: the header's
error code comes back and outputs, workspace and pads are untouched.

Outputs sit in arenas of their own (4 KiB pads, fill 0xFF) at their type's alignment where the header makes that the rule (the
guided, matting, temporal and flow families: "a pointer off its type's alignment") and at the documented 8 / 16 bytes elsewhere.
tests/test_ws_guard_host.py shows on the CPU which faults these comparisons reject."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import cwct_any_ref as A                                               # noqa: E402
import cwct_ops_ref as O                                               # noqa: E402
import flow_ref as FR                                                  # noqa: E402
import guided_ref as GR                                                # noqa: E402
import matting_ref as MR                                               # noqa: E402
import temporal_ref as TR                                              # noqa: E402
import vgg_ref as VR                                                   # noqa: E402
from ws_guard import PATTERNS, Arena, describe                         # noqa: E402

pytestmark = pytest.mark.gpu

OK, E_ARG, E_SHAPE, E_MODE, E_WORKSPACE = 0, -1, -2, -3, -4      # include/vstnet.h
OUT_PAD = 4096


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """a HIP error is sticky: nothing more is started on the card once a call has failed"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                            # noqa: BLE001
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def lib():
    from vstnet_amd import _lib
    return _lib.lib()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def vp(x):
    """a pointer argument from an address, a tensor, an Out / In, or None"""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, int):
        return C.c_void_p(x)
    if torch.is_tensor(x):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ptr)


def size_of(fn, *args):
    """the byte count of a size function that reports through a size_t* (the others return it)"""
    n = C.c_size_t(0)
    assert fn(*args, C.byref(n)) == OK, (fn.__name__, args)
    return int(n.value)


class Out:
    """an output of `shape` x `dtype` in an arena of its own at `align`; reset() refills it with 0xFF (and `init`, for an output
    that is also read: the factor's info)"""

    def __init__(self, shape, dtype, align, init=None):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.arena = Arena(int(np.prod(self.shape)) * self.dtype.itemsize, align, "cuda", pad=OUT_PAD)
        self.ptr = self.arena.ptr
        self.init = None if init is None else torch.from_numpy(np.ascontiguousarray(init, dtype=self.dtype).view(np.uint8).reshape(-1))
        self.reset()

    def reset(self):
        self.arena.fill(0xFF)
        if self.init is not None:
            self.arena.ws().copy_(self.init)

    def read(self):
        return np.frombuffer(self.arena.ws().cpu().numpy().tobytes(), dtype=self.dtype).reshape(self.shape)

    def untouched(self):
        return bool((self.arena.ws() == 0xFF).all())


class In:
    """an input on the device, with the bytes it must still hold afterwards"""

    def __init__(self, a):
        self.host = np.ascontiguousarray(a)
        self.t = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = self.t.data_ptr()

    def unchanged(self):
        return self.t.cpu().numpy().tobytes() == self.host.tobytes()


SEEN = []                         # (family, case, bytes, touched) of every case run, for the record


def contract(family, what, nbytes, align, call, outs, ins, verify, siblings=(), pad=65536):
    """the five assertions on one call.  call(ws_address) -> return code; siblings: (name, call) that dirty the arena first;
    verify(*outputs of the 0xFF run)"""
    arenas = {p: Arena(nbytes, align, "cuda", pad=pad) for p in PATTERNS}
    runs = []

    def one(arena, label):
        for o in outs:
            o.reset()
        rc = call(arena.ptr)
        assert rc == OK, (what, label, rc, lib().vst_error_string(rc))
        torch.cuda.synchronize()
        arena.check(f"{what} [{label}] workspace")                                                   # (a)
        for k, o in enumerate(outs):
            o.arena.check(f"{what} [{label}] output {k}")
        runs.append((label, [o.read() for o in outs]))

    for p in PATTERNS:
        arenas[p].fill(p)
        one(arenas[p], f"fill {p:#04x}")
    rng = arenas[0xFF].touched(arenas[0x7F])
    one(arenas[0x7F], "its own last run's workspace")
    for name, sib in siblings:
        rc = sib(arenas[0x7F].ptr)
        assert rc == OK, (what, name, rc)
        torch.cuda.synchronize()
        arenas[0x7F].check(f"{what}: sibling {name}")
        one(arenas[0x7F], f"after {name}")
    print(f"workspace {family}: {what}: {describe(nbytes, rng)} ({len(runs)} runs)")
    SEEN.append((family, what, nbytes, rng))
    first = runs[0][1]
    for label, got in runs[1:]:                                                                     # (b)
        for k, (a, b) in enumerate(zip(first, got)):
            assert a.tobytes() == b.tobytes(), (what, f"output {k} under [{label}] differs from the run under fill 0xff")
    verify(*first)                                                                                  # (c)
    assert rng is None or (0 <= rng[0] and rng[1] < nbytes), (what, rng, nbytes)                   # (d)
    for k, i in enumerate(ins):                                                                     # (e)
        assert i.unchanged(), (what, f"input {k} changed")
    return arenas


def refused(what, call, want_rc, arena, outs):
    """a refusal: the stated code, and nothing written anywhere.  call() -> return code"""
    arena.fill(0x7F)
    for o in outs:
        o.reset()
    rc = call()
    torch.cuda.synchronize()
    assert rc == want_rc, (what, rc, want_rc)
    arena.check(f"{what} (refused)")
    assert bool((arena.ws() == 0x7F).all()), (what, "a refused call wrote into the workspace")
    for k, o in enumerate(outs):
        o.arena.check(f"{what} (refused) output {k}")
        if o.init is None:
            assert o.untouched(), (what, f"a refused call wrote output {k}")


# ================================================================================================================ temporal
# (8, 8): one workgroup.  (128, 260): 17 workgroups of 2048 pixels, the last one ragged (512 pixels).
TEMPORAL_SIZES = ((8, 8), (128, 260))


@functools.lru_cache(maxsize=None)
def temporal_inputs(h, w):
    valid = (np.random.default_rng(h + w).random((h, w)) < 0.7).astype(np.uint8)
    valid[0, 0] = 255
    return dict(a8=TR.make_frame_u8(h, w, 0), b8=TR.make_frame_u8(h, w, 1), af=TR.make_frame_f32(h, w, 0),
                bf=TR.make_frame_f32(h, w, 1), flow=TR.make_flow(h, w, "real"), valid=valid)


def temporal_call(entry, d, h, w, with_flow, loss, warped):
    """-> call(ws) of one of the three L1 entry points on device inputs d"""
    L = lib()
    flow = d["flow"] if with_flow else None
    if entry == "u8":
        return lambda ws: L.vst_temporal_l1_u8(vp(d["a8"]), vp(d["b8"]), vp(flow), h, w, vp(loss), vp(warped), vp(ws), stream())
    if entry == "f32":
        return lambda ws: L.vst_temporal_l1_f32(vp(d["af"]), vp(d["bf"]), vp(flow), h, w, vp(loss), vp(warped), vp(ws), stream())
    return lambda ws: L.vst_temporal_l1_masked_u8(vp(d["a8"]), vp(d["b8"]), vp(flow), vp(d["valid"]), h, w, vp(loss), vp(warped),
                                                  vp(ws), stream())


@pytest.mark.parametrize("h,w", TEMPORAL_SIZES)
@pytest.mark.parametrize("with_flow", (True, False), ids=("flow+warped", "plain"))
@pytest.mark.parametrize("entry", ("u8", "f32", "masked"))
def test_temporal(entry, with_flow, h, w):
    host = temporal_inputs(h, w)
    d = {k: In(v) for k, v in host.items()}
    nbytes = size_of(lib().vst_temporal_workspace_bytes, h, w)
    flow = host["flow"] if with_flow else None
    loss = Out((4 if entry == "masked" else 3,), np.float64, 8)
    if entry == "f32":
        warped = Out((3, h, w), np.float32, 4)
    else:
        warped = Out((h, w, 3), np.uint8, 1)
    outs = [loss] + ([warped] if with_flow else [])
    # the siblings write losses and warps of their own
    sib_loss, sib_w8, sib_wf = Out((4,), np.float64, 8), Out((h, w, 3), np.uint8, 1), Out((3, h, w), np.float32, 4)
    siblings = [(f"vst_temporal_l1_{e}", temporal_call(e, d, h, w, True, sib_loss, sib_wf if e == "f32" else sib_w8))
                for e in ("u8", "f32", "masked") if e != entry]

    def verify(got_loss, got_warp=None):
        if entry == "u8":                           # bit-equal to the exact integer statement
            assert got_loss.tobytes() == TR.l1_u8(host["a8"], host["b8"], flow)[1].tobytes()
        elif entry == "masked":
            assert got_loss.tobytes() == FR.l1_masked_u8(host["a8"], host["b8"], flow, host["valid"])[1].tobytes()
        else:                                       # h w fp64 additions of non-negative terms
            want = TR.l1_f32(host["af"], host["bf"], flow)
            assert (np.abs(got_loss - want) / want <= h * w * 2.0 ** -53).all()
        if got_warp is not None:                    # the warp, outside the near ties of tests/test_gpu_temporal.py::test_warp
            tie = TR.near_tie(flow, h, w)
            if entry == "f32":
                same = (got_warp.view(np.uint32) == TR.warp_f32(host["af"], flow).view(np.uint32)).all(axis=0)
            else:
                same = (got_warp == TR.warp_u8(host["a8"], flow)).all(axis=2)
            assert tie.mean() <= 1e-3 and (same | tie).all()

    contract("temporal", f"vst_temporal_l1_{entry} {h}x{w} {'flow+warped' if with_flow else 'plain'}", nbytes, 8,
             temporal_call(entry, d, h, w, with_flow, loss, warped if with_flow else None), outs, list(d.values()), verify, siblings)
    for o in (sib_loss, sib_w8, sib_wf):
        o.arena.check("a sibling's output")
    assert nbytes == 24 * ((h * w + 2047) // 2048)    # three 8-byte partials per workgroup of 2048 pixels, and nothing else
    if not with_flow:
        assert warped.untouched()


# =============================================================================================================== fake flow
# the two smallest sizes of temporal_ref.SIZES; tables of w gw + h gh = 40 and 116 doubles, row buffers of 32 and 120: none a
# multiple of the 256 entries one workgroup fills
FAKE_FLOW_CASES = ((8, 8, 2, 3, 3), (12, 20, 3, 4, 5))


@pytest.mark.parametrize("h,w,gh,gw,ksize", FAKE_FLOW_CASES)
def test_fake_flow(h, w, gh, gw, ksize):
    assert (h, w) in TR.SIZES[:2] and (w * gw + h * gh) % 256 and (2 * gh * w) % 256
    L = lib()
    grid = np.random.default_rng(900 + h + w).normal(0.0, 8.0, (gh, gw, 2))
    shifts = (3.0, -7.0)
    nbytes = size_of(L.vst_fake_flow_workspace_bytes, h, w, gh, gw, ksize)
    g, flow = In(grid), Out((2, h, w), np.float32, 4)

    def verify(got):
        want = TR.fake_flow(grid, shifts, h, w, ksize)
        tol = 0.5 * float(np.spacing(np.float32(np.abs(want).max()))) + 1e-12
        assert np.abs(got.astype(np.float64) - want).max() <= tol

    contract("fake flow", f"vst_fake_flow {h}x{w} grid {gh}x{gw} ksize {ksize}", nbytes, 8,
             lambda ws: L.vst_fake_flow(vp(g), gh, gw, shifts[0], shifts[1], ksize, vp(flow), h, w, vp(ws), stream()),
             [flow], [g], verify)


# ==================================================================================================================== flow
# "tiny" 8x8 with one level; "t2" 61x83 with 3; "t3" 96x128 with 4, which crosses the 32 x 32 tile's seams; radius 1 and 3
FLOW_CASES = (("tiny", 1, 1, 1), ("tiny", 1, 3, 3), ("t2", 3, 1, 1), ("t2", 3, 3, 3), ("t3", 4, 1, 1), ("t3", 4, 3, 3))


@pytest.mark.parametrize("kind,levels,iters,radius", FLOW_CASES)
def test_flow(kind, levels, iters, radius):
    from test_gpu_flow import pair, want_flow
    L = lib()
    ref, src = pair(kind)
    h, w = ref.shape[:2]
    nbytes = size_of(L.vst_flow_workspace_bytes, h, w, levels)
    r, s = In(ref), In(src)
    fwd, bwd, valid = Out((2, h, w), np.float32, 4), Out((2, h, w), np.float32, 4), Out((h, w), np.uint8, 1)

    def call(ws):
        """the estimator both ways in one workspace, then the consistency mask of the two fields"""
        rc = L.vst_flow_lk_u8(vp(r), vp(s), h, w, levels, iters, radius, 1e-3, vp(fwd), vp(ws), stream())
        rc = rc or L.vst_flow_lk_u8(vp(s), vp(r), h, w, levels, iters, radius, 1e-3, vp(bwd), vp(ws), stream())
        return rc or L.vst_flow_consistency(vp(fwd), vp(bwd), h, w, vp(valid), stream())

    def verify(got_f, got_b, got_v):
        for got, swap in ((got_f, False), (got_b, True)):             # one fp32 ulp at max(|v|, 1); at most 1e-3 differ at all
            want = want_flow(kind, levels, iters, radius, swap)
            ulp = np.spacing(np.maximum(np.abs(want), np.float32(1.0)))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
            assert int((got != want).sum()) <= 1e-3 * got.size
        want_v, margin = FR.consistency(got_f, got_b)
        close = margin < 1e-9
        assert close.mean() < 1e-3 and ((got_v == want_v) | close).all() and set(np.unique(got_v)) <= {0, 1}

    contract("flow", f"vst_flow_lk_u8 x 2 + vst_flow_consistency {kind} {h}x{w} levels {levels} iters {iters} radius {radius}",
             nbytes, 8, call, [fwd, bwd, valid], [r, s], verify)


# ================================================================================================================== guided
# the first case of guided_ref.CASES (24 x 36) and the first with another working size that is no multiple of 16 (12 x 16, at
# the largest radius); one eps
GUIDED_CASES = (GR.CASES[0], GR.CASES[2])


@pytest.mark.parametrize("work_hw,full_hw,r", GUIDED_CASES)
def test_guided(work_hw, full_hw, r):
    from test_gpu_guided import check_f32, check_u8
    L = lib()
    eps = GR.EPS[0]
    G, P, S, ref = GR.case(work_hw, full_hw, r, eps)
    (h, w), (H, W) = work_hw, full_hw
    assert h % 16 or w % 16
    nbytes = size_of(L.vst_guided_workspace_bytes, h, w, r)
    g, p, s = In(G), In(P), In(S)
    other = In(np.ascontiguousarray(-P[::-1]))                        # the sibling fit's target
    coef, out8, outf = Out((12, h, w), np.float32, 4), Out((H, W, 3), np.uint8, 1), Out((3, H, W), np.float32, 4)
    sib_coef = Out((12, h, w), np.float32, 4)

    def call(ws):
        rc = L.vst_guided_fit(vp(g), vp(p), h, w, r, eps, vp(coef), vp(ws), stream())
        rc = rc or L.vst_guided_apply_u8(vp(coef), h, w, vp(s), H, W, vp(out8), stream())
        return rc or L.vst_guided_apply_f32(vp(coef), h, w, vp(s), H, W, vp(outf), stream())

    def verify(_, got8, gotf):
        what = f"{work_hw}->{full_hw} r={r} eps={eps}"
        check_f32(gotf, ref, what)
        check_u8(got8, ref, what)

    sibling = ("vst_guided_fit of another frame",
               lambda ws: L.vst_guided_fit(vp(g), vp(other), h, w, r, GR.EPS[1], vp(sib_coef), vp(ws), stream()))
    contract("guided", f"vst_guided_fit + applies {h}x{w}->{H}x{W} r={r}", nbytes, 8, call, [coef, out8, outf], [g, p, s], verify,
             [sibling])
    sib_coef.arena.check("the sibling's coefficients")


# ================================================================================================================= matting
# (3, 3, 1): the smallest, one tile.  (3, 40, 1): the first of matting_ref.CASES with several tiles (16 wide) and a ragged last
# one.  (37, 53, 1) adds rows of tiles, ragged both ways.
MATTING_CASES = ((3, 3, 1), (3, 40, 1), (37, 53, 1))


@pytest.mark.parametrize("h,w,r", MATTING_CASES)
@pytest.mark.parametrize("grad", (True, False), ids=("grad", "loss only"))
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
def test_matting(u8, grad, h, w, r):
    from test_gpu_matting import check
    assert (h, w, r) in MR.CASES
    L = lib()
    G, X, ref = MR.case(h, w, r, "noise", u8)
    Gs, Xs, _ = MR.case(h, w, r, "noise", not u8)
    nbytes = size_of(L.vst_matting_workspace_bytes, h, w, r)
    g, x, xs = In(G), In(X), In(Xs)
    loss, gr = Out((3,), np.float64, 8), Out((3, h, w), np.float32, 4)
    sl, sg = Out((3,), np.float64, 8), Out((3, h, w), np.float32, 4)
    fn, other = (L.vst_matting_loss_u8, L.vst_matting_loss_f32) if u8 else (L.vst_matting_loss_f32, L.vst_matting_loss_u8)

    def verify(got_loss, got_grad=None):
        check(got_loss, got_grad, ref, f"{h}x{w} r={r} {'u8' if u8 else 'f32'}")

    siblings = [("the same entry " + ("without" if grad else "with") + " the gradient",
                 lambda ws: fn(vp(g), vp(x), h, w, r, MR.EPS, vp(sl), None if grad else vp(sg), vp(ws), stream())),
                ("the other entry with the gradient",
                 lambda ws: other(vp(g), vp(xs), h, w, r, MR.EPS, vp(sl), vp(sg), vp(ws), stream())),
                ("the other entry without the gradient",
                 lambda ws: other(vp(g), vp(xs), h, w, r, MR.EPS, vp(sl), None, vp(ws), stream()))]
    contract("matting", f"vst_matting_loss_{'u8' if u8 else 'f32'} {h}x{w} r={r} {'grad' if grad else 'loss only'}", nbytes, 8,
             lambda ws: fn(vp(g), vp(x), h, w, r, MR.EPS, vp(loss), vp(gr) if grad else None, vp(ws), stream()),
             [loss] + ([gr] if grad else []), [g, x, xs], verify, siblings)
    if not grad:
        assert gr.untouched(), "the gradient buffer was written though no pointer to it was passed"
    sl.arena.check("a sibling's loss")
    sg.arena.check("a sibling's gradient")


# ===================================================================================================================== VGG
E53 = 2.0 ** -53
MSE_SPAN = 1024                   # csrc/vgg.hip vgg_mse: one workgroup per 1024 elements (count + 1023) / 1024, 256 threads x 4
VGG_FRAMES = ((9, 9), (37, 53))   # the minimum; odd at every pool (37x53 -> 19x27 -> 10x14 -> 5x7)


@pytest.fixture(scope="module")
def encoder():
    from vstnet_amd.vgg import VGGEncoder
    return VGGEncoder(VR.weights(), "cuda:0")


@functools.lru_cache(maxsize=None)
def vgg_frame_refs(h, w):
    """the frame and the records of vgg_ref's fp64 and fp32 encoders, in the layout of the golden file that vgg_ref.ratios reads"""
    img = VR.image_u8(h, w, 300 + h)
    sd = VR.weights()
    key = f"{h}x{w}"
    with torch.no_grad():
        gold = {f"{key}.rec_f64": VR.records(VR.encode(VR.planar(img, torch.float64), sd)).numpy(),
                f"{key}.rec_f32": VR.records(VR.encode(VR.planar(img, torch.float32), sd)).numpy()}
    return img, gold, key


@pytest.mark.parametrize("h,w", VGG_FRAMES)
@pytest.mark.parametrize("with_map", (True, False), ids=("relu4_1", "records only"))
@pytest.mark.parametrize("entry", ("u8", "f32"))
def test_vgg_features(encoder, entry, with_map, h, w):
    from vstnet_amd.vgg import level_sizes
    L = lib()
    img, gold, key = vgg_frame_refs(h, w)
    frame = In(img if entry == "u8" else np.ascontiguousarray(np.moveaxis(img, 2, 0).astype(np.float32) / np.float32(255)))
    nbytes = size_of(L.vst_vgg_workspace_bytes, h, w)
    h4, w4 = level_sizes(h, w)[3]
    rec, fmap = Out((VR.RECORD_OFFSETS[3] + 1024,), np.float64, 8), Out((h4 * w4, 512), np.float32, 16)
    fn = L.vst_vgg_features_u8 if entry == "u8" else L.vst_vgg_features_f32
    outs = [rec] + ([fmap] if with_map else [])

    def run(ws, size):
        return fn(encoder._plan, vp(frame), h, w, vp(rec), vp(fmap) if with_map else None, vp(ws), size, stream())

    def verify(got_rec, got_map=None):
        r = VR.ratios({"rec": got_rec}, gold, key)                    # the bound of tests/test_gpu_vgg.py, on the eight record groups
        assert max(r.values()) <= VR.FACTOR, (key, r)
        if got_map is not None:       # the fourth record's means are this very map's: the bound of test_gpu_vgg_ops.py::test_mean_std
            v, n = got_map.astype(np.float64), got_map.shape[0]
            assert np.isfinite(v).all()
            assert (np.abs(v.sum(axis=0) / n - got_rec[896:896 + 512]) <= (n + 8) * E53 * np.abs(v).sum(axis=0) / n).all()

    arenas = contract("VGG", f"vst_vgg_features_{entry} {h}x{w} {'with relu4_1' if with_map else 'records only'}", nbytes, 16,
                      lambda ws: run(ws, nbytes), outs, [frame], verify)
    if not with_map:
        assert fmap.untouched()
    a = arenas[0x7F]
    refused("one byte short", lambda: run(a.ptr, nbytes - 1), E_WORKSPACE, a, [rec, fmap])
    refused("an 8-byte address", lambda: run(a.ptr + 8, nbytes), E_WORKSPACE, a, [rec, fmap])


@pytest.mark.parametrize("n,c", ((2, 64), (1961, 128)))               # one chunk; 31 chunks of 64 rows, the last of 41
def test_vgg_mean_std(n, c):
    L = lib()
    x = torch.randn((n, c), generator=torch.Generator().manual_seed(n + c)).numpy()
    x[:, 1] += 100.0
    x[:, 2] = 0.0
    xin, out = In(x), Out((2, c), np.float64, 8)
    nbytes = size_of(L.vst_vgg_mean_std_workspace_bytes, n, c)

    def run(ws, size):
        return L.vst_vgg_mean_std(vp(xin), n, c, VR.EPS, vp(out), vp(ws), size, stream())

    def verify(got):                                                  # the bounds of tests/test_gpu_vgg_ops.py::test_mean_std
        v = x.astype(np.float64)
        mean = v.sum(axis=0) / n
        var = ((v - mean) ** 2).sum(axis=0) / (n - 1)
        std = np.sqrt(var + VR.EPS)
        assert (np.abs(got[0] - mean) <= (n + 8) * E53 * np.abs(v).sum(axis=0) / n).all()
        assert (np.abs(got[1] - std) <= (n + 8) * E53 * (var + VR.EPS) / (2 * std)).all()

    arenas = contract("VGG", f"vst_vgg_mean_std n={n} C={c}", nbytes, 8, lambda ws: run(ws, nbytes), [out], [xin], verify)
    a = arenas[0x7F]
    refused("one byte short", lambda: run(a.ptr, nbytes - 1), E_WORKSPACE, a, [out])
    refused("a 4-byte address", lambda: run(a.ptr + 4, nbytes), E_WORKSPACE, a, [out])


@pytest.mark.parametrize("count", (1, 2 * MSE_SPAN + 452))            # one element; three workgroups, the last one ragged
def test_vgg_mse(count):
    from vstnet_amd import _lib
    L = lib()
    assert count == 1 or count % MSE_SPAN
    g = torch.Generator().manual_seed(count)
    a, b = torch.randn(count, generator=g).numpy(), (torch.randn(count, generator=g) + 3.0).numpy()
    ain, bin_, out = In(a), In(b), Out((1,), np.float64, 8)

    def verify(got):                                                  # the bound of tests/test_gpu_vgg_ops.py::test_mse
        d2 = (a.astype(np.float64) - b.astype(np.float64)) ** 2
        assert abs(got[0] - d2.sum() / count) <= (count + 8) * E53 * d2.sum() / count

    contract("VGG", f"vst_vgg_mse_f64 count={count}", _lib.VGG_MSE_WS_BYTES, 256,
             lambda ws: L.vst_vgg_mse_f64(vp(ain), vp(bin_), count, vp(out), vp(ws), stream()), [out], [ain, bin_], verify)


# =============================================================================================================== cWCT fp32
# One L per regime of cwct_ops_ref.stats_groups: "512" at 516 (two workgroups, the second of 4 pixels) and at 1729 (L % 4 != 0:
# the scalar loads); "1024", "2048" and "capped" are reached by STATS_LONG alone, each once, at N = 32.
STATS_CASES = [(N, L) for N in (32, 64, 128) for L in (516, 1729)] + [(32, L) for L in O.STATS_LONG]
assert sorted({O.stats_groups(L)[2] for _, L in STATS_CASES}) == ["1024", "2048", "512", "capped"]


def check_record(got, r32, want, N, L):
    r = O.stats_ratio(got, r32, want, N, skip=A.skip_ch(N))[0]
    assert got[0] == L and r <= O.FACTOR["stats"], (N, L, r)


@pytest.mark.parametrize("N,L", STATS_CASES)
def test_cwct_stats(N, L):
    Lb = lib()
    if L in O.STATS_LONG:
        x = O.long_input(L)
        want = O.stats64_chunked(x)
    else:
        x = O.stats_input(N, L, "scales")
        want = O.stats64(x)
    xin, rec = In(x), Out((O.rec_len(N),), np.float64, 256)
    nbytes = int(Lb.vst_cwct_stats_workspace_bytes(N, L))

    def verify(got):
        check_record(got, O.stats32(x), want, N, L)

    contract("cWCT fp32", f"vst_cwct_stats N={N} L={L} [{O.stats_groups(L)[2]}]", nbytes, 256,
             lambda ws: Lb.vst_cwct_stats(vp(xin), N, L, None, 0, vp(rec), vp(ws), stream()), [rec], [xin], verify)


@pytest.mark.parametrize("N,L", [(N, L) for N in (32, 64, 128) for L in O.PLAN_L])
def test_cwct_stats_labels(N, L):
    """the plan form at the tables' two lengths (1092 = 2 workgroups + 68 pixels, 1729: L % 4 != 0), KRES + 1 slots: two passes"""
    from vstnet_amd.cwct import ops
    Lb = lib()
    n = O.KRES[N] + 1
    x = O.plan_input(N, L)
    cm, sm = O.plan_mask(L, n, "runs", N)
    xin, cmin = In(x), In(cm)
    plan = ops.label_plan(cmin.t, torch.from_numpy(sm).cuda())
    lut = ops.plan_info(plan)[2]
    plan_before = plan.cpu().numpy().tobytes()
    out = Out((O.MAX_SLOTS, O.rec_len(N)), np.float64, 256)
    nbytes = int(Lb.vst_cwct_labels_workspace_bytes(N, L))

    def verify(got):
        want, r32 = O.stats_labels64(x, cm, lut, n), O.stats_labels32(x, cm, lut, n, 0)
        for s in range(n):
            assert got[s, 0] == want[s, 0]
            assert O.stats_ratio(got[s], r32[s], want[s], N, skip=(O.CONST_CH,))[0] <= O.FACTOR["stats"], (N, L, s)

    contract("cWCT fp32", f"vst_cwct_stats_labels N={N} L={L} slots={n}", nbytes, 256,
             lambda ws: Lb.vst_cwct_stats_labels(vp(xin), N, L, vp(cmin), vp(plan), 0, vp(out), vp(ws), stream()), [out],
             [xin, cmin], verify)
    assert plan.cpu().numpy().tobytes() == plan_before


# =============================================================================================================== cWCT code
# the smallest frame of the code tests per sp_steps, and one whose row count is no multiple of the rows one workgroup takes
# (cwct_ops_ref.code_groups: 24 x 40 -> 960 rows in groups of 256; 48 x 80 -> 960 rows in groups of 128 ... checked below)
CODE_CASES = ((2, 8, 8), (2, 24, 40), (1, 16, 16), (1, 48, 80))


@pytest.mark.parametrize("sp,H,W", CODE_CASES)
def test_cwct_stats_code(sp, H, W):
    from vstnet_amd.cwct import ops
    Lb = lib()
    assert (sp, H, W, None) in O.CODE_CASES
    rows_n, per = O.code_groups(H, W, sp)
    if (H, W) not in ((8, 8), (16, 16)):
        assert rows_n % per and rows_n > per
    z = O.code_input(sp, H, W)
    code = ops.z_to_code(torch.from_numpy(z).cuda(), H, W, sp)
    rows = code.cpu().numpy().reshape(-1, z.shape[0])
    cin = In(rows)
    N = z.shape[0]
    rec = Out((O.rec_len(N),), np.float64, 256)
    nbytes = int(Lb.vst_cwct_stats_code_workspace_bytes(H, W, sp))

    def verify(got):
        const = int(np.nonzero((rows == O.CONST_VAL).all(0))[0][0])
        inside = np.ones(rows.shape[0], dtype=bool)
        want = O.stats64(rows.T, inside)
        r32 = O.stats32(np.ascontiguousarray(rows.T), inside.astype(np.uint8), 1, groups=(-(-rows_n // per), per, "code"))
        assert got[0] == rows.shape[0] and O.stats_ratio(got, r32, want, N, skip=(const,))[0] <= O.FACTOR["stats"]

    contract("cWCT code", f"vst_cwct_stats_code sp_steps={sp} {H}x{W}", nbytes, 256,
             lambda ws: Lb.vst_cwct_stats_code(vp(cin), H, W, sp, vp(rec), vp(ws), stream()), [rec], [cin], verify)


@pytest.mark.parametrize("H,W,n", ((24, 40, 3), (72, 104, 9)))
def test_cwct_stats_labels_code(H, W, n):
    from vstnet_amd.cwct import ops
    Lb = lib()
    assert (H, W, n, None) in O.CODE_LABEL_CASES
    z = O.code_input(2, H, W)
    code = ops.z_to_code(torch.from_numpy(z).cuda(), H, W, 2)
    rows = code.cpu().numpy().reshape(-1, 32)
    mask = O.code_label_mask(H, W, n)
    dmask = torch.from_numpy(mask).cuda()
    plan = ops.label_plan(dmask, dmask)
    lut = ops.plan_info(plan)[2]
    mrows = ops.mask_to_code(dmask, H, W).cpu().numpy()
    cin, min_ = In(rows), In(mrows)
    out = Out((O.MAX_SLOTS, O.rec_len(32)), np.float64, 256)
    nbytes = int(Lb.vst_cwct_stats_labels_code_workspace_bytes(H, W))

    def verify(got):
        Lr, per = O.labels_code_groups(H, W)
        xt = np.ascontiguousarray(rows.T)
        want = O.stats_labels64(xt, mrows, lut, n)
        r32 = O.stats_labels32(xt, mrows, lut, n, n, groups=(-(-Lr // per), per, "code"))
        const = int(np.nonzero((rows == O.CONST_VAL).all(0))[0][0])
        for s in range(n):
            assert got[s, 0] == want[s, 0]
            assert O.stats_ratio(got[s], r32[s], want[s], 32, skip=(const,))[0] <= O.FACTOR["stats"], (H, W, s)

    contract("cWCT code", f"vst_cwct_stats_labels_code {H}x{W} slots={n}", nbytes, 256,
             lambda ws: Lb.vst_cwct_stats_labels_code(vp(cin), H, W, vp(min_), vp(plan), n, vp(out), vp(ws), stream()), [out],
             [cin, min_], verify)


# ================================================================================================= cWCT fp64 and any width
ANY_N = (1, 5, 48, 200, 256)
L_N = 516                         # fp32 `_n`: two workgroups of 512 pixels, the second of 4
L_64 = A.CHUNK + 1                # fp64: two chunks of 2048 pixels, the second of 1


def sized_refusals(what, run, nbytes, align, arena, outs):
    """run(ws, size): one byte short -> VST_E_WORKSPACE; a null workspace -> VST_E_WORKSPACE; nothing written either time"""
    refused(f"{what}: one byte short", lambda: run(arena.ptr, nbytes - 1), E_WORKSPACE, arena, outs)
    refused(f"{what}: no workspace", lambda: run(None, nbytes), E_WORKSPACE, arena, outs)


@pytest.mark.parametrize("N", ANY_N)
def test_cwct_stats_n(N):
    Lb = lib()
    x = A.stats_input_n(N, L_N, "scales")
    xin, rec = In(x), Out((O.rec_len(N),), np.float64, 256)
    nbytes = int(Lb.vst_cwct_stats_n_workspace_bytes(N, L_N))

    def run(ws, size):
        return Lb.vst_cwct_stats_n(vp(xin), N, L_N, None, 0, vp(rec), vp(ws), size, stream())

    arenas = contract("cWCT any width", f"vst_cwct_stats_n N={N} L={L_N}", nbytes, 256, lambda ws: run(ws, nbytes), [rec], [xin],
                      lambda got: check_record(got, O.stats32(x), O.stats64(x), N, L_N))
    sized_refusals("vst_cwct_stats_n", run, nbytes, 256, arenas[0x7F], [rec])


def check_record64(got, x, N, L):
    r = A.stats64_ratio(got, A.stats_e64(x), A.stats_ld(x), N, skip=A.skip_ch(N))[0]
    assert got[0] == L and r <= A.FACTOR64, (N, L, r)


@pytest.mark.parametrize("N", ANY_N)
def test_cwct_stats_n_f64(N):
    Lb = lib()
    x = A.stats_input_n(N, L_64, "scales")
    xin, rec = In(x), Out((O.rec_len(N),), np.float64, 256)
    nbytes = int(Lb.vst_cwct_stats_n_f64_workspace_bytes(N, L_64))

    def run(ws, size):
        return Lb.vst_cwct_stats_n_f64(vp(xin), N, L_64, None, 0, vp(rec), vp(ws), size, stream())

    arenas = contract("cWCT fp64", f"vst_cwct_stats_n_f64 N={N} L={L_64}", nbytes, 256, lambda ws: run(ws, nbytes), [rec], [xin],
                      lambda got: check_record64(got, x, N, L_64))
    sized_refusals("vst_cwct_stats_n_f64", run, nbytes, 256, arenas[0x7F], [rec])


@pytest.mark.parametrize("N", A.F64_N["f64"])
def test_cwct_stats_f64(N):
    Lb = lib()
    x = A.stats_input_n(N, L_64, "scales")
    xin, rec = In(x), Out((O.rec_len(N),), np.float64, 256)
    nbytes = int(Lb.vst_cwct_stats_f64_workspace_bytes(N, L_64))
    contract("cWCT fp64", f"vst_cwct_stats_f64 N={N} L={L_64}", nbytes, 256,
             lambda ws: Lb.vst_cwct_stats_f64(vp(xin), N, L_64, None, 0, vp(rec), vp(ws), stream()), [rec], [xin],
             lambda got: check_record64(got, x, N, L_64))


def factor_args(N, k):
    content, styles, al = O.factor_input(N, k, 1e4)
    cin, sins = In(content), [In(s) for s in styles]
    ptrs = (C.c_void_p * k)(*[s.ptr for s in sins])
    alphas = (C.c_float * k)(*[float(a) for a in al])
    info = Out((2 + k,), np.int32, 256, init=np.zeros(2 + k, np.int32))
    return content, styles, al, cin, sins, ptrs, alphas, info


# (the existing tables leave out 8 styles at N = 256, and so does this one)
FACTOR_ANY = [(N, k) for N in ANY_N for k in (1, 8) if not (N == 256 and k == 8)]
AC = 0.3


@pytest.mark.parametrize("N,k", FACTOR_ANY)
def test_cwct_factor_n(N, k):
    Lb = lib()
    content, styles, al, cin, sins, ptrs, alphas, info = factor_args(N, k)
    aff = Out((N * N + N,), np.float32, 256)
    nbytes = int(Lb.vst_cwct_factor_n_workspace_bytes(N))

    def run(ws, size):
        return Lb.vst_cwct_factor_n(vp(cin), ptrs, alphas, k, AC, O.EPS, N, vp(aff), vp(info), vp(ws), size, stream())

    def verify(got, got_info):
        a32, info32 = O.factor32(content, styles, al, AC, N)
        ref = O.factor64(content, styles, al, AC, N, info32)
        assert got_info.tolist() == info32
        assert O.ratio("factor", O.factor_err(got, ref, N), O.factor_err(a32, ref, N)) <= O.FACTOR["factor"]

    pre, pinfo = Out((O.rec_len(N),), np.float64, 256), Out((1,), np.int32, 256, init=np.zeros(1, np.int32))
    sibling = ("vst_cwct_prefactor_n", lambda ws: Lb.vst_cwct_prefactor_n(vp(sins[0]), N, O.EPS, vp(pre), vp(pinfo), vp(ws), nbytes,
                                                                          stream()))
    arenas = contract("cWCT any width", f"vst_cwct_factor_n N={N} styles={k}", nbytes, 256, lambda ws: run(ws, nbytes), [aff, info],
                      [cin] + sins, verify, [sibling])
    sized_refusals("vst_cwct_factor_n", run, nbytes, 256, arenas[0x7F], [aff, info])


@pytest.mark.parametrize("N", ANY_N)
def test_cwct_prefactor_n(N):
    Lb = lib()
    content, styles, al, cin, sins, ptrs, alphas, info = factor_args(N, 1)
    pre, pinfo = Out((O.rec_len(N),), np.float64, 256), Out((1,), np.int32, 256, init=np.zeros(1, np.int32))
    aff = Out((N * N + N,), np.float32, 256)
    nbytes = int(Lb.vst_cwct_factor_n_workspace_bytes(N))

    def run(ws, size):
        return Lb.vst_cwct_prefactor_n(vp(sins[0]), N, O.EPS, vp(pre), vp(pinfo), vp(ws), size, stream())

    def verify(got, got_info):
        """what tests/test_gpu_cwct_ops_any.py::test_factor_n asserts of a prefactored record: its head, and that the factor
        gives the unfactored record's affine bit for bit"""
        assert got_info.tolist() == [0] and got[0] == -(styles[0][0] + 1.0) and got[1:1 + N].tobytes() == styles[0][1:1 + N].tobytes()
        ws = Arena(nbytes, 256, "cuda").fill(0x00)
        both = []
        for rec in (sins[0], In(got)):
            p1 = (C.c_void_p * 1)(rec.ptr)
            aff.reset(), info.reset()
            assert Lb.vst_cwct_factor_n(vp(cin), p1, alphas, 1, AC, O.EPS, N, vp(aff), vp(info), vp(ws), nbytes, stream()) == OK
            torch.cuda.synchronize()
            both.append(aff.read().tobytes())
        assert both[0] == both[1]

    sibling = ("vst_cwct_factor_n", lambda ws: Lb.vst_cwct_factor_n(vp(cin), ptrs, alphas, 1, AC, O.EPS, N, vp(aff), vp(info), vp(ws),
                                                                    nbytes, stream()))
    arenas = contract("cWCT any width", f"vst_cwct_prefactor_n N={N}", nbytes, 256, lambda ws: run(ws, nbytes), [pre, pinfo],
                      [cin] + sins, verify, [sibling])
    sized_refusals("vst_cwct_prefactor_n", run, nbytes, 256, arenas[0x7F], [pre, pinfo])


def verify_factor64(content, styles, al, N):
    def verify(got, got_info):
        a64, info64 = A.factor_e64(content, styles, al, AC, N)
        ref = A.factor_ld(content, styles, al, AC, N, info64)
        assert got_info.tolist() == info64
        assert A.ratio64(O.factor_err(got, ref, N), O.factor_err(a64, ref, N)) <= A.FACTOR64
    return verify


@pytest.mark.parametrize("N,k", FACTOR_ANY)
def test_cwct_factor_n_f64(N, k):
    Lb = lib()
    content, styles, al, cin, sins, ptrs, alphas, info = factor_args(N, k)
    aff = Out((N * N + N,), np.float64, 256)
    nbytes = int(Lb.vst_cwct_factor_n_f64_workspace_bytes(N))

    def run(ws, size):
        return Lb.vst_cwct_factor_n_f64(vp(cin), ptrs, alphas, k, AC, O.EPS, N, vp(aff), vp(info), vp(ws), size, stream())

    arenas = contract("cWCT fp64", f"vst_cwct_factor_n_f64 N={N} styles={k}", nbytes, 256, lambda ws: run(ws, nbytes), [aff, info],
                      [cin] + sins, verify_factor64(content, styles, al, N))
    sized_refusals("vst_cwct_factor_n_f64", run, nbytes, 256, arenas[0x7F], [aff, info])


@pytest.mark.parametrize("N,k", [(N, k) for N in A.F64_N["f64"] for k in (1, 8)])
def test_cwct_factor_f64(N, k):
    Lb = lib()
    content, styles, al, cin, sins, ptrs, alphas, info = factor_args(N, k)
    aff = Out((N * N + N,), np.float64, 256)
    nbytes = int(Lb.vst_cwct_factor_f64_workspace_bytes(N))
    contract("cWCT fp64", f"vst_cwct_factor_f64 N={N} styles={k}", nbytes, 256,
             lambda ws: Lb.vst_cwct_factor_f64(vp(cin), ptrs, alphas, k, AC, O.EPS, N, vp(aff), vp(info), vp(ws), stream()),
             [aff, info], [cin] + sins, verify_factor64(content, styles, al, N))


# ============================================================================================================= deep resize
# deep_resize_ref.SHAPES: 42x56 -> 40x56 is one horizontal pass (the size function says 0 bytes: nothing may be touched at all),
# 97x55 -> 64x36 one step of two passes, 160x140 -> 12x10 -> 12x8 two steps
DEEP_SHAPES = ((42, 56, 64), (97, 55, 64), (160, 140, 12))


@pytest.mark.parametrize("Ws,Hs,max_size", DEEP_SHAPES)
def test_deep_resize(Ws, Hs, max_size):
    import deep_resize_ref as DR
    from vstnet_amd.yuv import DeepImgResize, _device_planes
    L = lib()
    assert (Ws, Hs, max_size) in DR.SHAPES
    spec = DR.DeepYuvSpec("420mpeg2", "bt709", "limited", 10)
    flat = DR.random_planes(spec, Hs, Ws, 1000 + Ws)
    fin = In(flat)
    rs = DeepImgResize((Hs, Ws), spec, max_size, DR.DOWN_SCALE, "cuda")          # the tables and the step list; its own buffer is not used
    w, h = rs.size_wh
    nbytes = size_of(L.vst_yuv16_img_resize_workspace_bytes, Hs, Ws, len(rs.steps), rs._steps)
    assert (nbytes == 0) == (rs.work is None)
    y, u, v = _device_planes(fin.t, Hs, Ws, spec, "test")
    lay, mat, rng_, depth = spec.codes
    outf, out8 = Out((3, h, w), np.float32, 4), Out((h, w, 3), np.uint8, 1)

    def call(ws):
        return L.vst_yuv16_img_resize_f32(vp(y), vp(u), vp(v), Hs, Ws, depth, lay, mat, rng_, len(rs.steps), rs._steps,
                                          vp(rs.tables), vp(ws) if nbytes else None, vp(outf), vp(out8), stream())

    def verify(got, twin):                                            # tests/test_gpu_deep_resize.py::resize_case
        want = DR.reference(flat, Hs, Ws, spec, max_size)
        assert np.abs(got.transpose(1, 2, 0).astype(np.float64) - want).max() <= DR.kernel_tolerance((Ws, Hs), max_size)
        assert got.min() >= 0.0 and got.max() <= 1.0 and not (twin != DR.twin_of(got.transpose(1, 2, 0))).any()

    tables_before = None if rs.tables is None else rs.tables.cpu().numpy().tobytes()
    contract("deep resize", f"vst_yuv16_img_resize_f32 {Ws}x{Hs} -> {w}x{h} ({len(rs.steps)} steps)", nbytes, 256, call,
             [outf, out8], [fin], verify)
    assert tables_before is None or rs.tables.cpu().numpy().tobytes() == tables_before


# ================================================================================================================== passes
# 32 x 48 with B = 1 and B = 2, both sp_steps, all four precisions; the float and the u8 end of every entry point in one test.
# Yardstick: the oracle comparison of tests/test_gpu_parity.py::test_network_vs_oracle_ragged (assert_close under NET_TOL) on
# the float end; the u8 end of a forward pass is held to the same oracle, the u8 end of an inverse pass is cpu_ref.to_uint8 of
# the float end's output, bit for bit (test_uint8_frame_edge).  The decode forms get an affine map per image: plain decode a
# random map near the identity, which the oracle side applies to z in fp64; _labels, _blend and _mix the identity (one-hot
# weights for _mix), under which every one of them is the plain inverse of the same code.
PH, PW = 32, 48
PASS_MODES = ("fp32", "bf16x3", "f16x2", "f16x2h")
_NETS, _ORACLE = {}, {}


def pass_net(sp, prec):
    import test_gpu_parity as parity
    key = (sp, prec)
    if key not in _NETS:
        _NETS[key] = parity.make_net("photo" if sp == 2 else "art", prec)
    net, sd, _ = _NETS[key]
    return net._ensure_packed(torch.device("cuda", torch.cuda.current_device())), sd


def pass_oracle(sp, B, H=PH, W=PW):
    """frames, x = ToTensor(frames), the oracle's z, a perturbed z' with a map near the identity per image, and the oracle's
    inverse of z' and of the mapped z': made once per (sp_steps, B)"""
    from oracle import cpu_ref
    key = (sp, B, H, W)
    if key not in _ORACLE:
        _, sd = pass_net(sp, "fp32")
        g = torch.Generator().manual_seed(11 + sp + 10 * B)
        frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
        x = frames.permute(0, 3, 1, 2).float().div(255).contiguous()
        N = 32 if sp == 2 else 128
        with torch.no_grad():
            zr = cpu_ref.revnet_forward(x, sd, sp)
            zp = (zr + 0.03 * torch.randn(zr.shape, generator=g)).contiguous()
            T = torch.eye(N, dtype=torch.float64) + 0.05 * torch.randn((B, N, N), generator=g, dtype=torch.float64) / N ** 0.5
            t0 = 0.02 * torch.randn((B, N), generator=g, dtype=torch.float64)
            aff = torch.cat([T.reshape(B, -1), t0], dim=1).float().contiguous()
            Tf, tf = aff[:, :N * N].reshape(B, N, N).double(), aff[:, N * N:].double()
            zm = (torch.einsum("bnm,bmhw->bnhw", Tf, zp.double()) + tf[:, :, None, None]).float()
            _ORACLE[key] = dict(frames=frames.numpy(), x=x.numpy(), zr=zr, zp=zp.numpy(), aff=aff.numpy(),
                                yr=cpu_ref.revnet_inverse(zp, sd, sp), ym=cpu_ref.revnet_inverse(zm, sd, sp))
    return _ORACLE[key]


def code_of(z, H, W, sp):
    """[B, 32 H W] packed codes of z (numpy), image by image"""
    from vstnet_amd.cwct import ops
    return np.stack([ops.z_to_code(torch.from_numpy(np.ascontiguousarray(zb)).cuda(), H, W, sp).cpu().numpy() for zb in z])


def z_of(code, B, H, W, sp):
    L = lib()
    c = torch.from_numpy(np.ascontiguousarray(code)).cuda()
    z = torch.empty((B, 32, H, W) if sp == 2 else (B, 128, H // 2, W // 2), dtype=torch.float32, device="cuda")
    assert L.vst_code_to_z(vp(c), vp(z), B, H, W, sp, stream()) == OK
    return z.cpu()


PASS_ENTRIES = ("forward", "inverse", "encode", "decode", "decode_blend", "decode_mix")


@pytest.mark.parametrize("prec", PASS_MODES)
@pytest.mark.parametrize("sp", (2, 1))
@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("entry", PASS_ENTRIES)
def test_passes(entry, B, sp, prec):
    from oracle import cpu_ref
    from test_gpu_parity import NET_TOL, assert_close
    from vstnet_amd import _lib
    L = lib()
    H, W = PH, PW
    w, _ = pass_net(sp, prec)
    P = _lib.PRECISIONS[prec]
    o = pass_oracle(sp, B)
    N = 32 if sp == 2 else 128
    rows = H * W if sp == 2 else H * W // 4
    zshape = (B, 32, H, W) if sp == 2 else (B, 128, H // 2, W // 2)
    packed = entry not in ("forward", "inverse")
    nbytes = int(L.vst_pass_workspace_bytes(1 if packed else B, H, W))
    what = f"vst_revnet_{entry}" + "{} " + f"{H}x{W} B={B} sp_steps={sp} {prec}"
    rng = np.random.default_rng(B + sp)
    if entry in ("forward", "encode"):
        x, frames = In(o["x"]), In(o["frames"])
        zf, z8 = Out(zshape, np.float32, 256), Out(zshape, np.float32, 256)

        def verify(got):
            z = torch.from_numpy(got.copy()) if entry == "forward" else z_of(got.reshape(B, -1), B, H, W, sp)
            assert_close(z, o["zr"], NET_TOL[prec], what.format(""))

        if entry == "forward":
            ff = lambda ws: L.vst_revnet_forward(C.byref(w), vp(x), vp(zf), vp(ws), B, 3, H, W, sp, P, stream())       # noqa: E731
            f8 = lambda ws: L.vst_revnet_forward_u8(C.byref(w), vp(frames), vp(z8), vp(ws), B, H, W, sp, P, stream())   # noqa: E731
        else:
            ff = lambda ws: L.vst_revnet_encode(C.byref(w), vp(x), vp(zf), vp(ws), B, 3, H, W, P, stream())            # noqa: E731
            f8 = lambda ws: L.vst_revnet_encode_u8(C.byref(w), vp(frames), vp(z8), vp(ws), B, H, W, P, stream())        # noqa: E731
        contract("passes", what.format(""), nbytes, 256, ff, [zf], [x], verify, [("the u8 end", f8)])
        contract("passes", what.format("_u8"), nbytes, 256, f8, [z8], [frames], verify, [("the float end", ff)])
        return
    yf, y8 = Out((B, 3, H, W), np.float32, 256), Out((B, H, W, 3), np.uint8, 256)
    if entry == "inverse":
        src, extra, want = In(o["zp"]), [], o["yr"]
        ff = lambda ws: L.vst_revnet_inverse(C.byref(w), vp(src), vp(yf), vp(ws), B, 3, H, W, sp, P, stream())          # noqa: E731
        f8 = lambda ws: L.vst_revnet_inverse_u8(C.byref(w), vp(src), vp(y8), vp(ws), B, H, W, sp, P, stream())          # noqa: E731
    else:
        src = In(code_of(o["zp"], H, W, sp))
        ident = np.concatenate([np.eye(N, dtype=np.float32).reshape(-1), np.zeros(N, np.float32)])
        if entry == "decode":
            aff, want = In(o["aff"]), o["ym"]
            extra, mid = [aff], (vp(aff),)
        elif entry == "decode_blend":
            aff, st = In(np.tile(ident, (B, 1))), In(rng.random((B, rows)).astype(np.float32))
            extra, mid, want = [aff, st], (vp(aff), vp(st)), o["yr"]
        else:                                                         # decode_mix: K = 2, one-hot weights per row
            pick = rng.integers(0, 2, (B, 1, rows)).astype(np.float32)
            aff, wr = In(np.tile(ident, (B, 2, 1))), In(np.concatenate([pick, 1.0 - pick], axis=1))
            extra, mid, want = [aff, wr], (vp(aff), 2, vp(wr), None), o["yr"]
        fn = getattr(L, f"vst_revnet_{entry}")
        fn8 = getattr(L, f"vst_revnet_{entry}_u8")
        ff = lambda ws: fn(C.byref(w), vp(src), *mid, vp(yf), vp(ws), B, 3, H, W, sp, P, stream())                      # noqa: E731
        f8 = lambda ws: fn8(C.byref(w), vp(src), *mid, vp(y8), vp(ws), B, H, W, sp, P, stream())                        # noqa: E731
    floats = []

    def verify_f(got):
        floats.append(torch.from_numpy(got.copy()))
        assert_close(floats[0], want, NET_TOL[prec], what.format(""))

    def verify_8(got):
        assert np.array_equal(got, cpu_ref.to_uint8(floats[0]).numpy()), "the u8 end is not to_uint8 of the float end"

    contract("passes", what.format(""), nbytes, 256, ff, [yf], [src] + extra, verify_f, [("the u8 end", f8)])
    contract("passes", what.format("_u8"), nbytes, 256, f8, [y8], [src] + extra, verify_8, [("the float end", ff)])


@pytest.mark.parametrize("prec", PASS_MODES)
def test_passes_decode_labels(prec):
    """one image (the call takes no batch), photorealistic codes only: two slots, the identity map in each"""
    from oracle import cpu_ref
    from test_gpu_parity import NET_TOL, assert_close
    from vstnet_amd import _lib
    from vstnet_amd.cwct import ops
    L = lib()
    H, W, sp = PH, PW, 2
    w, _ = pass_net(sp, prec)
    P = _lib.PRECISIONS[prec]
    o = pass_oracle(sp, 1)
    mask = O.code_label_mask(H, W, 2)
    dmask = torch.from_numpy(mask).cuda()
    plan = ops.label_plan(dmask, dmask)
    assert ops.plan_info(plan)[0] == 2
    mrows = In(ops.mask_to_code(dmask, H, W).cpu().numpy())
    ident = np.concatenate([np.eye(32, dtype=np.float32).reshape(-1), np.zeros(32, np.float32)])
    aff, src = In(np.tile(ident, (O.MAX_SLOTS, 1))), In(code_of(o["zp"], H, W, sp))
    yf, y8 = Out((1, 3, H, W), np.float32, 256), Out((1, H, W, 3), np.uint8, 256)
    nbytes = int(L.vst_pass_workspace_bytes(1, H, W))
    ff = lambda ws: L.vst_revnet_decode_labels(C.byref(w), vp(src), vp(aff), vp(mrows), vp(plan), 2, vp(yf), vp(ws), 3, H, W, P,   # noqa: E731
                                               stream())
    f8 = lambda ws: L.vst_revnet_decode_labels_u8(C.byref(w), vp(src), vp(aff), vp(mrows), vp(plan), 2, vp(y8), vp(ws), H, W, P,   # noqa: E731
                                                  stream())
    what = "vst_revnet_decode_labels{} " + f"{H}x{W} {prec}"
    floats = []

    def verify_f(got):
        floats.append(torch.from_numpy(got.copy()))
        assert_close(floats[0], o["yr"], NET_TOL[prec], what.format(""))

    def verify_8(got):
        assert np.array_equal(got, cpu_ref.to_uint8(floats[0]).numpy())

    contract("passes", what.format(""), nbytes, 256, ff, [yf], [src, aff, mrows], verify_f, [("the u8 end", f8)])
    contract("passes", what.format("_u8"), nbytes, 256, f8, [y8], [src, aff, mrows], verify_8, [("the float end", ff)])


def test_passes_sub_batch_remainder():
    """B = 3 at the frame tests/test_gpu_pass_blocks.py finds, with 1 < vst_pass_sub_batch < B: the pass loop ends on a remainder.
    Forward and inverse, float ends, bf16x3.  Yardstick: that test's own - every value finite, inverse(forward(x)) within 1e-2."""
    from test_gpu_pass_blocks import _sub_batch_frame
    from vstnet_amd import _lib
    L = lib()
    B = 3
    H, W = _sub_batch_frame(L, B)
    assert 1 < L.vst_pass_sub_batch(B, H, W) < B
    w, _ = pass_net(2, "bf16x3")
    P = _lib.PRECISIONS["bf16x3"]
    x = In(torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5)).numpy())
    z, y = Out((B, 32, H, W), np.float32, 256), Out((B, 3, H, W), np.float32, 256)
    nbytes = int(L.vst_pass_workspace_bytes(B, H, W))
    zs = []

    def verify_z(got):
        assert np.isfinite(got).all()
        zs.append(In(got))

    contract("passes", f"vst_revnet_forward {H}x{W} B={B} bf16x3 (sub-batch {L.vst_pass_sub_batch(B, H, W)})", nbytes, 256,
             lambda ws: L.vst_revnet_forward(C.byref(w), vp(x), vp(z), vp(ws), B, 3, H, W, 2, P, stream()), [z], [x], verify_z)

    def verify_y(got):
        assert np.isfinite(got).all() and float(np.abs(got - x.host).max()) < 1e-2

    contract("passes", f"vst_revnet_inverse {H}x{W} B={B} bf16x3 (sub-batch {L.vst_pass_sub_batch(B, H, W)})", nbytes, 256,
             lambda ws: L.vst_revnet_inverse(C.byref(w), vp(zs[0]), vp(y), vp(ws), B, 3, H, W, 2, P, stream()), [y], [zs[0]], verify_y)


# ================================================================================================================ the record
def test_every_family_of_the_header_was_run():
    """runs last in this module: with the whole module selected, every family above has left its lines"""
    want = {"temporal", "fake flow", "flow", "guided", "matting", "VGG", "cWCT fp32", "cWCT code", "cWCT any width", "cWCT fp64",
            "passes", "deep resize"}
    seen = {f for f, _, _, _ in SEEN}
    if len(SEEN) >= 100:          # (a selection of this module leaves fewer lines and is not judged)
        assert seen == want, want - seen
