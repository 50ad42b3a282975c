"""Per-frame style maps on the GPU ("Style maps per frame"): vst_style_frame against its numpy restatement
and against the static route (cWCT.bind_style_map of the host's weights), the zero-sum flag, and cWCT.frame_style_map's
checks.  No tolerance anywhere: every comparison is on float32 bit patterns."""
import numpy as np
import pytest
import torch

from tests import style_frames_ref as ref
from tests.zc import ptr, stream
from vstnet_amd import _lib

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SIZES = [(8, 8), (12, 20), (64, 72)]        # the smallest legal; cells no multiple of anything; 288 cells: two workgroups, one ragged


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """a HIP error is sticky: nothing more is started on the card once a call has failed"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                            # noqa: BLE001
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def code_shape(sp, H, W):
    return (1, 32, H, W) if sp == 2 else (1, 128, H // 2, W // 2)


def run_kernel(planes, sp, dense=True, rows=True, flag=0):
    """(dense [K,n] int32 bit patterns, rows [K,n], the flag word afterwards), device tensors; outputs poisoned first"""
    P, H, W = planes.shape
    K, n = max(P, 2), (H * W if sp == 2 else H * W // 4)
    dp = T(planes).cuda()
    dd = torch.full((K, n), -7.0, device="cuda") if dense else None
    dr = torch.full((K, n), -7.0, device="cuda") if rows else None
    df = torch.full((1,), flag, dtype=torch.int32, device="cuda")
    p = lambda t: ptr(t) if t is not None else None        # noqa: E731
    _lib.check(_lib.lib().vst_style_frame(ptr(dp), P, p(dd), p(dr), ptr(df), H, W, sp, stream()), "vst_style_frame")
    view = lambda t: None if t is None else t.view(torch.int32)      # noqa: E731
    return view(dd), view(dr), int(df.item())


def want_of(planes, sp):
    """the restatement's (dense, rows) as int32 bit patterns on the device, and its flag"""
    P, H, W = planes.shape
    w, flagged = ref.style_frame(planes, sp)
    dense = T(ref.bits(w.reshape(w.shape[0], -1)).view(np.int32)).cuda()
    rows = T(ref.bits(np.stack([ref.rows_of(p, H, W, sp) for p in w])).view(np.int32)).cuda()
    return dense, rows, flagged


_wants = {}


def cached_want(P, H, W, sp):
    key = (P, H, W, sp)
    if key not in _wants:
        planes = ref.planes_of(P, H, W, 1000 * P + H + sp, lo=1)
        _wants[key] = (planes,) + want_of(planes, sp)
    return _wants[key]


# ------------------------------------------------------------------------------------------------ 1. kernel, bit for bit
@pytest.mark.parametrize("sp", [2, 1])
@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_equals_the_restatement(sp, P, H, W):
    planes, dense, rows, flagged = cached_want(P, H, W, sp)
    assert not flagged
    d, r, f = run_kernel(planes, sp)
    assert f == 0 and torch.equal(d, dense) and torch.equal(r, rows)
    d_only, none, f = run_kernel(planes, sp, rows=False)
    assert none is None and f == 0 and torch.equal(d_only, dense)
    none, r_only, f = run_kernel(planes, sp, dense=False)
    assert none is None and f == 0 and torch.equal(r_only, rows)
    # rows = vst_map_to_code(dense), the library's own permutation, plane by plane
    df = d.view(torch.float32)
    back = torch.empty_like(df)
    for k in range(df.shape[0]):
        _lib.check(_lib.lib().vst_map_to_code(ptr(df[k]), ptr(back[k]), H, W, sp, stream()), "vst_map_to_code")
    assert torch.equal(back.view(torch.int32), r)


@pytest.mark.parametrize("sp", [2, 1])
def test_every_pair_of_two_planes(sp):
    """every (v, total) pair of K = 2 and every byte of the ramp (tests/test_style_frames_host.py has the same planes)"""
    y, x = np.mgrid[0:256, 0:256]
    planes = np.stack([y, x]).astype(np.uint8)
    planes[1, 0, 0] = 1
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    if sp == 1:
        planes, ramp = (np.repeat(np.repeat(a, 2, 1), 2, 2) for a in (planes, ramp))
    for a in (np.ascontiguousarray(planes), np.ascontiguousarray(ramp)):
        dense, rows, flagged = want_of(a, sp)
        d, r, f = run_kernel(a, sp)
        assert not flagged and f == 0 and torch.equal(d, dense) and torch.equal(r, rows)


# ------------------------------------------------------------------------------------------------ 2. the static route
@pytest.mark.parametrize("sp", [2, 1])
@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_kernel_equals_bind_style_map(sp, P):
    """the planes through the shipped host route (PIL BOX, utils.style_map_weights) and cWCT.bind_style_map"""
    from PIL import Image
    from models.cWCT import cWCT
    from utils.utils import style_map_weights
    H, W = 12, 20
    planes = cached_want(P, H, W, sp)[0]
    imgs = [Image.fromarray(p) for p in planes]
    if sp == 1:
        imgs = [im.resize((W // 2, H // 2), Image.BOX) for im in imgs]
    host = style_map_weights([np.asarray(im, dtype=np.uint8) for im in imgs])
    bound = cWCT().bind_style_map(host, code_shape(sp, H, W), "cuda")
    got = cWCT.frame_style_map(code_shape(sp, H, W), T(planes).cuda())
    assert got.K == bound.K == max(P, 2) and got.code_shape == bound.code_shape
    assert torch.equal(got.dense.view(torch.int32), bound.dense.view(torch.int32))
    assert torch.equal(got.rows.view(torch.int32), bound.rows.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. zero-sum pixels
@pytest.mark.parametrize("sp", [2, 1])
def test_zero_sum_pixels(sp):
    H, W, P = 12, 20, 3
    clean = cached_want(P, H, W, sp)[0]
    d0, r0, f = run_kernel(clean, sp, flag=0)
    assert f == 0
    assert run_kernel(clean, sp, flag=0x10)[2] == 0x10           # a clean frame touches no bit
    planes = clean.copy()
    if sp == 2:
        holes = [(1, 2), (9, 17)]                                # code pixels, in different cells
        for y, x in holes:
            planes[:, y, x] = 0
    else:
        holes = [(0, 1), (4, 8)]                                 # whole 2 x 2 blocks of zeros
        for y, x in holes:
            planes[:, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = 0
    dense, rows, flagged = want_of(planes, sp)
    assert flagged
    d, r, f = run_kernel(planes, sp, flag=0)
    assert f == 1 and torch.equal(d, dense) and torch.equal(r, rows)
    assert run_kernel(planes, sp, flag=0x10)[2] == 0x11          # OR, not store
    cW = W if sp == 2 else W // 2
    df, d0f = d.view(torch.float32).clone(), d0.view(torch.float32)
    assert bool(torch.isfinite(df).all())
    for y, x in holes:
        assert df[:, y * cW + x].tolist() == [1.0, 0.0, 0.0]
        df[:, y * cW + x] = d0f[:, y * cW + x]
    assert torch.equal(df.view(torch.int32), d0)                 # every other pixel is unchanged
    # the library call sets the caller's flag word too
    from models.cWCT import cWCT
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    cWCT.frame_style_map(code_shape(sp, H, W), T(planes).cuda(), flags=word)
    assert int(word.item()) == 1


# ------------------------------------------------------------------------------------------------ 4. the library call
def test_frame_style_map_checks_and_allocates_nothing():
    from models.cWCT import cWCT
    H, W = 12, 20
    shape = code_shape(2, H, W)
    planes = T(cached_want(3, H, W, 2)[0]).cuda()
    with pytest.raises(ValueError):
        cWCT.frame_style_map(shape, planes.float())
    with pytest.raises(ValueError):
        cWCT.frame_style_map(shape, planes.cpu())
    with pytest.raises(ValueError):
        cWCT.frame_style_map(shape, torch.zeros((9, H, W), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        cWCT.frame_style_map(shape, torch.zeros((3, H, W + 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        cWCT.frame_style_map(shape, planes.permute(0, 2, 1).contiguous().permute(0, 2, 1))       # not contiguous
    with pytest.raises(ValueError):
        cWCT.frame_style_map(shape, planes, out=cWCT.empty_style_map(shape, 2, "cuda"))          # a map of another K
    out = cWCT.empty_style_map(shape, 3, "cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = cWCT.frame_style_map(shape, planes, out=out, flags=word)
    assert torch.cuda.memory_allocated() == before
    assert got is out
    assert torch.equal(out.dense[0].view(torch.int32), cached_want(3, H, W, 2)[1])
