"""spmv_bcsr4<2> and spmv_bcsr4_tile<2> at the limits of their pipeline and of the x tile: the block patterns of
tests/bcsr4_row_cases.py through mi_bcsr4_spmv_dev and, expanded to CSR, through MI_KERNEL_BCSR4 — BITWISE against the oracle's block
chain (O.spmv_bcsr4; for the expanded matrix also O.spmv, the same bits).  No tolerance.

Every test first asserts mi_bcsr4_tile_probe's answer for its pattern (tests/test_bcsr4_row_limits.py does the same on the CPU), then
that the HANDLE holds and uses the lists accordingly (mi_bcsr4_tile_info, kernel_name).  Outputs start as NaN with NaN guard entries
behind them.  MI355_SPMV_AUTOTUNE=0, MI355_PLACEMENT_DRAWS=0, MI355_REORDER=0, MI355_BCSR_SELL=0: nothing is measured, no sliced copy."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bcsr4_row_cases as BC
from navierstokes_amd import mpk
from oracle import oracle as O
from test_gpu_edges import assert_same

pytestmark = pytest.mark.gpu
GUARD = 8
TILE_SETTINGS = (None, "0", "1")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


@pytest.fixture(autouse=True)
def _quiet(monkeypatch):
    for k in ("MI355_SPMV_AUTOTUNE", "MI355_PLACEMENT_DRAWS", "MI355_REORDER", "MI355_BCSR_SELL"):
        monkeypatch.setenv(k, "0")
    for k in ("MI355_STREAM_ROW_ALIGN", "MI355_SPMV_KERNEL", "MI355_TILE_NT", "MI355_STREAM_NT", "MI355_BCSR_TILE", "MI355_AUTO_BCSR",
              "MI355_BCSR_SELL_FORM"):
        monkeypatch.delenv(k, raising=False)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x, y) of a case: seeded x from (-1, 1) over the block columns, y = the oracle's blocked product — computed once, read-only"""
    K = BC.case(name)
    x = np.random.default_rng(8000).uniform(-1.0, 1.0, 4 * K.nbcols)
    y = O.spmv_bcsr4(K.ptrow, K.indcol, K.coef, x)
    assert np.isfinite(y).all()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def set_tile(monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("MI355_BCSR_TILE", raising=False)
    else:
        monkeypatch.setenv("MI355_BCSR_TILE", setting)


def lists_expected(K, setting):
    """(built, in_use) of mi_bcsr4_tile_info: the lists exist where the probe says so unless switched off, and run only when forced
    (nothing is measured here)"""
    probe = mpk.bcsr4_tile_probe(K.nbrows, K.ptrow, K.indcol)
    assert probe == K.probe, (probe, K.probe)
    built = probe["would_build"] and setting != "0"
    return int(built), int(built and setting == "1")


def guarded_product(run, n, want, what, offset=0):
    buf = torch.full((offset + n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    run(buf[offset:offset + n])
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert_same(h[offset:offset + n], want, what)
    assert np.isnan(h[:offset]).all() and np.isnan(h[offset + n:]).all(), f"{what}: wrote outside y"


@pytest.mark.parametrize("name", BC.ALL)
def test_blocked_handle_bitwise(name, monkeypatch):
    """mi_bcsr4_spmv_dev with MI355_BCSR_TILE unset, 0 and 1: (built, in_use) as the probe and the setting say — (1, 1) for the
    pattern at the cap under 1, (0, 0) one column over the cap and one block under the size whatever the setting"""
    K = BC.case(name)
    x, want = reference(name)
    dx = dev(x)
    for setting in TILE_SETTINGS:
        set_tile(monkeypatch, setting)
        expect = lists_expected(K, setting)
        if name in ("xtile_over", "xtile_small") or name.startswith("pipe"):
            assert expect == (0, 0)
        if name in ("xtile_cap", "xtile_exact") and setting == "1":
            assert expect == (1, 1)
        B = mpk.bcsr4x4_matrix(K.nbrows, K.ptrow, K.indcol, K.coef, nbcols=K.nbcols)
        built, in_use = ctypes.c_int(), ctypes.c_int()
        mpk.check(mpk.lib().mi_bcsr4_tile_info(B.handle, ctypes.byref(built), ctypes.byref(in_use), None, None))
        assert (built.value, in_use.value) == expect, (name, setting, built.value, in_use.value, expect)
        guarded_product(lambda y: mpk.SpMV_BCSR(y, dx, B), 4 * K.nbrows, want, f"{name} MI355_BCSR_TILE={setting}")
        B.close()


@functools.lru_cache(maxsize=None)
def expanded(name):
    K = BC.case(name)
    n, ncols, p, c, v = BC.to_csr(K)
    x, want = reference(name)
    assert_same(O.spmv(p, c, v, x), want, f"{name}: the CSR chain of the expanded matrix is the block chain")
    return n, ncols, p, c, v


@pytest.mark.parametrize("name,setting", [(nm, s) for nm in BC.ALL for s in (TILE_SETTINGS if nm.startswith("xtile") else (None,))])
def test_expanded_to_csr_and_forced_to_the_blocked_kernel(name, setting, monkeypatch):
    """the same pattern as a CSR matrix under MI_KERNEL_BCSR4: with a 16-byte aligned x the blocked copy runs (the kernel named says
    which form); with x one double into its buffer the blocked kernel's paired loads cannot be used and the product is
    spmv_csr_stream<1024, false> on the handle's table — the same bits either way"""
    K = BC.case(name)
    x, want = reference(name)
    n, ncols, p, c, v = expanded(name)
    set_tile(monkeypatch, setting)
    built, in_use = lists_expected(K, setting)
    S = mpk.rowblock_census(n, p, c, "stream")
    assert S["blocks"] >= 1 and S["long"] == 0
    A = mpk.csrmatrix(n, p, c, v, ncols=ncols).set_kernel("bcsr4")
    assert A.kernel_name() == ("spmv_bcsr4_tile<2>" if in_use else "spmv_bcsr4<2>"), (name, setting, A.kernel_name())
    dx = dev(x)
    assert dx.data_ptr() % 16 == 0
    guarded_product(lambda y: mpk.SpMV_CSR(y, dx, A), n, want, f"{name} expanded, aligned x, MI355_BCSR_TILE={setting}")
    xb = torch.full((ncols + 1,), float("nan"), dtype=torch.float64, device="cuda")
    xb[1:] = dx
    x8 = xb[1:]
    assert x8.data_ptr() % 16 == 8
    guarded_product(lambda y: mpk.SpMV_CSR(y, x8, A), n, want, f"{name} expanded, x 8-byte aligned: the stream kernel's table", offset=1)
    assert A.stream_info() == dict(nblk=S["blocks"], row_align=S["row_align"]), (A.stream_info(), S)
    A.close()
