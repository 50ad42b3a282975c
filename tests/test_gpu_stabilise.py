"""vstnet_amd.stabilise on the card against the numpy statement of the same formula (tests/stabilise_ref.py): every byte equal.  The
kernel uses only + - * /, comparisons and rint in fp64 without contraction, so a difference is a bug in one of the two statements,
not a tolerance."""
import numpy as np
import pytest
import torch

import stabilise_ref as S

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 7), (5, 1), (3, 4), (17, 19), (64, 96))      # 17 x 19: two workgroups of 256 pixels


def frames(h, w, seed):
    rng = np.random.default_rng(1000 * seed + 31 * h + w)
    cur_in = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    # the previous input is close to the current one over most of the frame (a weight worth having) and far from it elsewhere
    near = np.clip(cur_in.astype(np.int64) + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
    far = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    prev_in = np.where(rng.random((h, w, 1)) < 0.75, near, far)
    return cur_in, prev_in, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def flows(h, w):
    """name -> float32 [2,h,w]"""
    rng = np.random.default_rng(7 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = {"zero": np.zeros((2, h, w), np.float32),
           "whole": np.stack([np.full((h, w), 1.0), np.full((h, w), -1.0)]).astype(np.float32),
           "fractional": (rng.normal(0.0, 0.8, (2, h, w)) + np.array([0.3, -0.6])[:, None, None]).astype(np.float32),
           # samples that leave the frame on every side (and some that stay)
           "outward": (rng.normal(0.0, 1.0, (2, h, w)) * np.array([w, h])[:, None, None]).astype(np.float32),
           # every sample lands exactly on the last column and the last row; then exactly on the first
           "last": np.stack([xx - (w - 1), yy - (h - 1)]).astype(np.float32),
           "first": np.stack([xx, yy]).astype(np.float32)}
    odd = out["fractional"].copy().reshape(-1)
    vals = (np.nan, np.inf, -np.inf)
    for j in range(0, odd.size, 3):                 # a third of the entries: NaN, +inf, -inf in turn
        odd[j] = vals[(j // 3) % 3]
    out["nonfinite"] = odd.reshape(2, h, w)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def on_card(ci, pi, co, pw, flow, valid=None, **kw):
    from vstnet_amd.stabilise import stabilise
    out = stabilise(dev(ci), dev(pi), dev(co), dev(pw), dev(flow), None if valid is None else dev(valid), **kw)
    return out.cpu().numpy()


@pytest.mark.parametrize("h,w", SHAPES)
def test_every_byte(h, w):
    ci, pi, co, pw = frames(h, w, 0)
    valid = (np.random.default_rng(h + w).random((h, w)) < 0.7).astype(np.uint8) * 255
    for name, flow in flows(h, w).items():
        for v in (None, valid):
            want = S.stabilise(ci, pi, co, pw, flow, v)
            got = on_card(ci, pi, co, pw, flow, v)
            assert got.dtype == np.uint8 and got.shape == (h, w, 3)
            assert np.array_equal(got, want), (name, v is not None, int((got != want).sum()))
    # the blend does something: with a zero flow and the input unchanged nearly every byte moves towards prev_written
    moved = on_card(ci, ci, co, pw, np.zeros((2, h, w), np.float32))
    assert np.array_equal(moved, S.stabilise(ci, ci, co, pw, np.zeros((2, h, w), np.float32)))
    assert h * w == 1 or (moved != co).mean() > 0.5


@pytest.mark.parametrize("h,w", ((3, 4), (17, 19), (64, 96)))
def test_parameters(h, w):
    ci, pi, co, pw = frames(h, w, 1)
    fl = flows(h, w)["fractional"]
    assert np.array_equal(on_card(ci, pi, co, pw, fl, limit=0.0), co)           # limit 0: the frame as it came
    for kw in (dict(gain=1e-6), dict(gain=1.0 - 1e-12), dict(gain=0.999, limit=255.0), dict(sigma=1e-3), dict(sigma=1e6),
               dict(limit=0.5), dict(limit=1.5), dict(gain=0.31, sigma=2.5, limit=7.25)):
        want = S.stabilise(ci, pi, co, pw, fl, None, **{**S.DEFAULTS, **kw})
        assert np.array_equal(on_card(ci, pi, co, pw, fl, **kw), want), kw
        assert np.abs(want.astype(np.int64) - co).max() <= np.ceil({**S.DEFAULTS, **kw}["limit"])


def test_object_reused_on_one_stream():
    """A short recursion through one Stabiliser on a side stream, its output fed back: the bytes of the numpy recursion."""
    from vstnet_amd.stabilise import Stabiliser
    h, w, n = 17, 19, 5
    rng = np.random.default_rng(5)
    inputs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    outputs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    fl = [None] + [rng.normal(0.0, 1.0, (2, h, w)).astype(np.float32) for _ in range(1, n)]
    want = S.run_sequence(inputs, outputs, fl, gain=0.6, sigma=40.0, limit=30.0)
    st = Stabiliser((h, w), gain=0.6, sigma=40.0, limit=30.0)
    assert st.device == torch.device("cuda", torch.cuda.current_device())
    d_in, d_out, d_fl = [dev(a) for a in inputs], [dev(a) for a in outputs], [None] + [dev(a) for a in fl[1:]]
    ring = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    got = [outputs[0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        prev = d_out[0]
        for t in range(1, n):
            prev = st(d_in[t], d_in[t - 1], d_out[t], prev, d_fl[t], out=ring[t % 2])
            got.append(prev.clone())
        own = st(d_in[1], d_in[0], d_out[1], d_out[0], d_fl[1])                 # without `out`: the object's frame
        assert own is st.written
    stream.synchronize()
    for t in range(1, n):
        assert np.array_equal(got[t].cpu().numpy(), want[t]), t
    assert np.array_equal(own.cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="made for"):
        st(dev(np.zeros((8, 8, 3), np.uint8)), d_in[0], d_out[0], d_out[0], d_fl[1])


def test_argument_errors():
    from vstnet_amd import _lib
    from vstnet_amd.stabilise import stabilise
    h, w = 8, 12
    ci, pi, co, pw = (dev(a) for a in frames(h, w, 2))
    fl = torch.zeros((2, h, w), dtype=torch.float32, device="cuda")
    for kw in (dict(gain=0.0), dict(gain=1.0), dict(sigma=0.0), dict(limit=-1.0), dict(sigma=float("nan"))):
        with pytest.raises(ValueError):
            stabilise(ci, pi, co, pw, fl, **kw)
    for out in (pw, co, pi, ci):                    # never in place
        with pytest.raises(_lib.VstError):
            stabilise(ci, pi, co, pw, fl, out=out)
    with pytest.raises(ValueError):
        stabilise(ci, pi, co, pw, fl.cpu())
    with pytest.raises(ValueError):
        stabilise(ci, pi, co, pw, None)
    with pytest.raises(ValueError):
        stabilise(ci, pi, co, pw[:, :6].contiguous(), fl)
    with pytest.raises(ValueError):
        stabilise(ci, pi, co, pw, fl, valid=torch.ones((h, w), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        stabilise(ci.float(), pi, co, pw, fl)
    assert np.array_equal(stabilise(ci, pi, co, pw, fl).cpu().numpy(),
                          S.stabilise(ci.cpu().numpy(), pi.cpu().numpy(), co.cpu().numpy(), pw.cpu().numpy(), fl.cpu().numpy()))
