"""CPU: the width-generic cWCT (N = 1..256 outside the tuned {16, 32, 64, 128}; csrc/cwct_any.hip) — its exports are declared,
bound and built, its arguments are checked before any launch, and its route table is total.  No compute call is made."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

from vstnet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = [
    "vst_cwct_stats_n_workspace_bytes", "vst_cwct_stats_n", "vst_cwct_factor_n_workspace_bytes", "vst_cwct_factor_n",
    "vst_cwct_prefactor_n", "vst_cwct_apply_n", "vst_cwct_stats_n_f64_workspace_bytes", "vst_cwct_stats_n_f64",
    "vst_cwct_factor_n_f64_workspace_bytes", "vst_cwct_factor_n_f64", "vst_cwct_apply_n_f64",
]
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_new_exports_declared_bound_and_built(lib):
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    built = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3}
    for name in NEW_EXPORTS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.EXPORTS, name
        assert name in built, name
        assert hasattr(lib, name), name
    assert lib.vst_version() >= 103


def test_workspace_sizes_grow_with_width_and_length(lib):
    for fn in (lib.vst_cwct_stats_n_workspace_bytes, lib.vst_cwct_stats_n_f64_workspace_bytes):
        sizes = [fn(N, 1 << 16) for N in (1, 8, 48, 100, 256)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        lens = [fn(24, L) for L in (1, 1 << 12, 1 << 16, 1 << 20)]
        assert all(a < b for a, b in zip(lens, lens[1:])), lens
        assert fn(0, 1 << 16) == 0 and fn(257, 1 << 16) == 0
    for fn in (lib.vst_cwct_factor_n_workspace_bytes, lib.vst_cwct_factor_n_f64_workspace_bytes):
        sizes = [fn(N) for N in (1, 8, 48, 100, 256)]
        assert all(0 < a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert fn(0) == 0 and fn(257) == 0
    # the fp32 statistics record of the tuned kernels, per workgroup: n, shift[N], sum[N], co-moment[N*N]
    assert lib.vst_cwct_stats_n_workspace_bytes(48, 1 << 20) == 512 * (48 * 48 + 96 + 4) * 4


def test_argument_checks_before_any_launch(lib):
    """(every call below fails its checks: nothing is launched, so no GPU is needed)"""
    null = C.c_void_p(0)
    one = C.c_void_p(1)
    big = 1 << 40
    styles = (C.c_void_p * 1)(1)
    nostyle = (C.c_void_p * 1)(0)
    alphas = (C.c_float * 1)(1.0)
    for stats, ws_bytes in ((lib.vst_cwct_stats_n, lib.vst_cwct_stats_n_workspace_bytes),
                            (lib.vst_cwct_stats_n_f64, lib.vst_cwct_stats_n_f64_workspace_bytes)):
        for N in (0, 257, -3):
            assert stats(one, N, 100, null, 0, one, one, big, null) == E_SHAPE, N
        assert stats(null, 8, 100, null, 0, one, one, big, null) == E_ARG
        assert stats(one, 8, 100, null, 0, null, one, big, null) == E_ARG
        assert stats(one, 8, 0, null, 0, one, one, big, null) == E_ARG
        assert stats(one, 8, 100, null, 0, one, null, big, null) == E_WORKSPACE
        need = ws_bytes(48, 4096)
        assert stats(one, 48, 4096, null, 0, one, one, need - 1, null) == E_WORKSPACE
    for factor, ws_bytes in ((lib.vst_cwct_factor_n, lib.vst_cwct_factor_n_workspace_bytes),
                             (lib.vst_cwct_factor_n_f64, lib.vst_cwct_factor_n_f64_workspace_bytes)):
        for N in (0, 257):
            assert factor(one, styles, alphas, 1, 0.0, 2e-5, N, one, one, one, big, null) == E_SHAPE, N
        assert factor(null, styles, alphas, 1, 0.0, 2e-5, 8, one, one, one, big, null) == E_ARG
        assert factor(one, nostyle, alphas, 1, 0.0, 2e-5, 8, one, one, one, big, null) == E_ARG
        assert factor(one, styles, alphas, 1, 0.0, 2e-5, 8, null, one, one, big, null) == E_ARG
        assert factor(one, styles, alphas, 1, 0.0, 2e-5, 8, one, null, one, big, null) == E_ARG
        assert factor(one, styles, alphas, 0, 0.0, 2e-5, 8, one, one, one, big, null) == E_ARG
        assert factor(one, styles, alphas, 9, 0.0, 2e-5, 8, one, one, one, big, null) == E_ARG
        assert factor(one, styles, alphas, 1, 0.0, 2e-5, 8, one, one, null, big, null) == E_WORKSPACE
        assert factor(one, styles, alphas, 1, 0.0, 2e-5, 200, one, one, one, ws_bytes(200) - 1, null) == E_WORKSPACE
    pre, need = lib.vst_cwct_prefactor_n, lib.vst_cwct_factor_n_workspace_bytes(100)
    assert pre(one, 0, 2e-5, one, one, one, big, null) == E_SHAPE
    assert pre(one, 257, 2e-5, one, one, one, big, null) == E_SHAPE
    assert pre(null, 8, 2e-5, one, one, one, big, null) == E_ARG
    assert pre(one, 8, 2e-5, one, null, one, big, null) == E_ARG
    assert pre(one, 100, 2e-5, one, one, one, need - 1, null) == E_WORKSPACE
    for apply in (lib.vst_cwct_apply_n, lib.vst_cwct_apply_n_f64):
        assert apply(one, one, 0, 100, one, null, 0, null) == E_SHAPE
        assert apply(one, one, 257, 100, one, null, 0, null) == E_SHAPE
        assert apply(null, one, 8, 100, one, null, 0, null) == E_ARG
        assert apply(one, null, 8, 100, one, null, 0, null) == E_ARG
        assert apply(one, one, 8, 100, null, null, 0, null) == E_ARG
        assert apply(one, one, 8, 0, one, null, 0, null) == E_ARG
    # the tuned calls keep their contract
    assert lib.vst_cwct_apply(one, one, 48, 100, one, null, 0, null) == E_SHAPE


def test_width_route_table_is_total():
    from models.cWCT import cWCT
    seen = {cWCT.width_route(masked, dbl) for masked, dbl in itertools.product((False, True), (False, True))}
    assert seen == set(cWCT.WIDTH_ROUTES)
    assert not seen & set(cWCT.ROUTES)
    for masked, dbl in itertools.product((False, True), (False, True)):
        r = cWCT.width_route(masked, dbl)
        assert r.endswith("_f64") == dbl and ("masked" in r) == masked
    with pytest.raises(NotImplementedError):
        cWCT.route(False, False, 48)                # the tuned table is unchanged


def test_untuned_widths_outside_the_range_raise_before_touching_a_device():
    import torch
    from models.cWCT import cWCT
    cw = cWCT()
    for N in (257, 300):
        with pytest.raises(NotImplementedError):
            cw._route_of(torch.zeros(1, N, 2, 2), masked=False)
    cw._route_of(torch.zeros(1, 48, 2, 2), masked=True)
    assert cw.last_route == "any_width_masked_per_label"
    cw = cWCT(use_double=True)
    cw._route_of(torch.zeros(1, 8, 2, 2), masked=False)
    assert cw.last_route == "any_width_dense_f64"
