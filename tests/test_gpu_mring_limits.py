"""spmv_csr_mring at every limit of its plan: the matrices of tests/mring_cases.py through MI_KERNEL_MRING, BITWISE against the
oracle's fma chain in CSR order (O.spmv).  No tolerance.

Every test first asserts through mi_mring_plan_census that its matrix reaches the state it is named for, then that the handle runs
that plan (mring_info) and the instantiation kernel_name spells out.  Non-temporal value loads off and on (MI355_MRING_NT: the
multi-window ring has no setter); its staging layout follows the row lengths alone and is read from the name.  Outputs start as NaN
with NaN guard entries behind them.  MI355_SPMV_AUTOTUNE=0, MI355_PLACEMENT_DRAWS=0, MI355_REORDER=0: nothing depends on a timing."""
import functools

import numpy as np
import pytest
import torch

import mring_cases as MC
from navierstokes_amd import mpk
from oracle import oracle as O
from ring_cases import row_maps
from test_gpu_edges import assert_same
from test_ring_limits import check_want

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


@pytest.fixture(autouse=True)
def _quiet(monkeypatch):
    for k in ("MI355_SPMV_AUTOTUNE", "MI355_PLACEMENT_DRAWS", "MI355_REORDER"):
        monkeypatch.setenv(k, "0")
    monkeypatch.setenv("MI355_MRING", "1")
    for k in ("MI355_RING_ROW_ALIGN", "MI355_SPMV_KERNEL", "MI355_MRING_DEAL"):
        monkeypatch.delenv(k, raising=False)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=2)
def reference(name):
    K = MC.case(name)
    x = np.random.default_rng(8000).uniform(-1.0, 1.0, K.ncols)
    y = O.spmv(K.ptrow, K.indcol, K.coef, x)
    assert np.isfinite(y).all()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def run(name, monkeypatch, rowmap=None, ylen=None, mapped=False, streams=(None,)):
    K = MC.case(name)
    S = mpk.mring_plan_census(K.n, K.ptrow, K.indcol)
    check_want(S, K.want, name)
    x, want = reference(name)
    ylen = K.n if ylen is None else ylen
    rows = np.arange(K.n) if rowmap is None else rowmap.astype(np.int64)
    outside = np.ones(ylen + GUARD, bool)
    outside[rows] = False
    dx = dev(x)
    t = lambda b: "true" if b else "false"
    for nt in (0, 1):
        monkeypatch.setenv("MI355_MRING_NT", str(nt))
        A = mpk.csrmatrix(K.n, K.ptrow, K.indcol, K.coef, ncols=K.ncols, rowmap=rowmap)
        A.set_kernel("mring")
        info = A.mring_info()
        assert (info["built"], info["runs"], info["runs_not_served"], info["nt"]) == (True, S["runs"], S["runs_kind0"], bool(nt)), (info, S)
        nm = A.kernel_name()
        assert nm in [f"spmv_csr_mring<{MC.T}, {MC.NNZB}, {S['depth']}, {MC.MAX_B}, {t(mapped)}, {t(nt)}, {t(sk)}>" for sk in (0, 1)], nm
        for s in streams:
            buf = torch.full((ylen + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
            if s is None:
                mpk.SpMV_CSR(buf[:ylen], dx, A)
                torch.cuda.synchronize()
            else:
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    mpk.SpMV_CSR(buf[:ylen], dx, A)
                s.synchronize()
            h = buf.cpu().numpy()
            assert_same(h[rows], want, f"{name} nt={nt} stream={'null' if s is None else 'own'} ({nm})")
            assert np.isnan(h[outside]).all(), f"{name}: wrote outside its rows"
        A.close()


@pytest.mark.parametrize("name", MC.NAMES)
def test_case_bitwise(name, monkeypatch):
    """M1 to M6 on the null stream and on a stream of its own"""
    run(name, monkeypatch, streams=(None, torch.cuda.Stream()))


@pytest.mark.parametrize("name", ["m1", "m4", "m6", "m6_rect"])
def test_row_maps(name, monkeypatch):
    """rows scattered over a longer y (the MAPPED instantiation), rows moved up by an odd offset: what no row maps to stays NaN"""
    K = MC.case(name)
    for kind, rowmap, ylen in row_maps(K.n):
        run(name, monkeypatch, rowmap=rowmap, ylen=ylen, mapped=kind == "scattered")


def test_value_refresh(monkeypatch):
    """M4 after mi_csr_update_values: plain runs and PLAIN blocks read the CSR values, the loop the value stream"""
    K = MC.case("m4")
    x, _ = reference("m4")
    A = mpk.csrmatrix(K.n, K.ptrow, K.indcol, K.coef).set_kernel("mring")
    assert A.kernel_name().startswith("spmv_csr_mring<")
    for k, on_device in enumerate((False, True)):
        v = np.random.default_rng(950 + k).uniform(-1.0, 1.0, len(K.coef))
        A.update_values(dev(v) if on_device else v)
        y = torch.full((K.n,), float("nan"), dtype=torch.float64, device="cuda")
        mpk.SpMV_CSR(y, dev(x), A)
        assert_same(y, O.spmv(K.ptrow, K.indcol, v, x), f"m4 after refresh {k}")
