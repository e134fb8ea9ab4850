"""spmv_csr_stream<1024> and spmv_csr_tile<2048> at every limit of their row blocks: the matrices of tests/rowblock_cases.py through
MI_KERNEL_STREAM and MI_KERNEL_TILE, BITWISE against the oracle's fma chain in CSR order (O.spmv).  No tolerance.

Every test first asserts through mi_rowblock_census that its matrix reaches the branches it is named for
(tests/test_rowblock_limits.py does the same on the CPU), then that the HANDLE runs that table (mi_csr_stream_info / tile_info report
the census's blocks) with the instantiation asked for (kernel_name spells it out, SKEW included): a planner change that moves a case
off its limit, or a silent fallback, fails the test instead of emptying it.  Outputs start as NaN with NaN guard entries behind
them.  Nothing here depends on a timing: MI355_SPMV_AUTOTUNE=0, MI355_PLACEMENT_DRAWS=0, MI355_REORDER=0, MI355_BCSR_SELL=0."""
import functools

import numpy as np
import pytest
import torch

import rowblock_cases as RB
from navierstokes_amd import mpk
from oracle import oracle as O
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
    for k in ("MI355_SPMV_AUTOTUNE", "MI355_PLACEMENT_DRAWS", "MI355_REORDER", "MI355_BCSR_SELL"):
        monkeypatch.setenv(k, "0")
    for k in ("MI355_STREAM_ROW_ALIGN", "MI355_SPMV_KERNEL", "MI355_TILE_NT", "MI355_STREAM_NT"):
        monkeypatch.delenv(k, raising=False)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()      # (a copy: the cases' arrays are shared and read-only)


@functools.lru_cache(maxsize=None)
def reference(name, kern):
    """(x, y) of a case: seeded x from (-1, 1), y = the oracle's product — computed once, shared, read-only"""
    K = RB.case(name, kern)
    x = np.random.default_rng(9000 + RB.NNZBS[kern]).uniform(-1.0, 1.0, K.ncols)
    y = O.spmv(K.ptrow, K.indcol, K.coef, x)
    assert np.isfinite(y).all()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def name_of(kern, nt, skew):
    t = lambda b: "true" if b else "false"
    return f"spmv_csr_stream<1024, {t(nt)}>" if kern == "stream" else f"spmv_csr_tile<2048, {t(nt)}, {t(skew)}>"


def make(name, kern, monkeypatch, nt, rowmap=None):
    """the case as a handle on its kernel, with what every test asserts first: the census of the case, and that the handle runs that
    table with the instantiation asked for.  The tile kernel's kind of value loads is read when the handle is made (MI355_TILE_NT; the
    plan must exist by then: MI355_TILE=1), the stream kernel's is set on the handle."""
    K = RB.case(name, kern)
    S = mpk.rowblock_census(K.n, K.ptrow, K.indcol, kern)
    check_want(S, K.want, f"{name}, {kern}")
    if kern == "tile":
        check_want(S, K.want_tile, f"{name}, {kern}")
        monkeypatch.setenv("MI355_TILE", "1")
        monkeypatch.setenv("MI355_TILE_NT", str(nt))
    A = mpk.csrmatrix(K.n, K.ptrow, K.indcol, K.coef, ncols=K.ncols, rowmap=rowmap)
    A.set_kernel(kern)
    if kern == "tile":
        info = A.tile_info()
        assert (info["built"], info["nblk"], info["nt"]) == (True, S["blocks"], bool(nt)), (info, S)
    else:
        mpk.check(mpk.lib().mi_csr_set_nontemporal(A.handle, -1, nt))
        assert A.stream_info() == dict(nblk=S["blocks"], row_align=S["row_align"]), (A.stream_info(), S)
    assert A.kernel_name() == name_of(kern, nt, S["skew"]), A.kernel_name()
    return K, A, S


def product(K, A, x, want, what, ylen=None, rows=None, stream=None, offset=0):
    """y = A x: the oracle's bits in the rows of y, NaN everywhere else (the guard entries behind y included).  offset = 1: x and y
    are views one double into their buffers (8-byte aligned only)."""
    ylen = K.n if ylen is None else ylen
    rows = np.arange(K.n) if rows is None else rows
    xb = torch.full((K.ncols + offset,), float("nan"), dtype=torch.float64, device="cuda")
    xb[offset:] = dev(x)
    buf = torch.full((offset + ylen + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    dx, dy = xb[offset:], buf[offset:offset + ylen]
    assert dx.data_ptr() % 16 == 8 * offset and dy.data_ptr() % 16 == 8 * offset
    if stream is None:
        mpk.SpMV_CSR(dy, dx, A)
        torch.cuda.synchronize()
    else:
        torch.cuda.synchronize()                                         # x and buf were written on the null stream
        with torch.cuda.stream(stream):
            mpk.SpMV_CSR(dy, dx, A)
        stream.synchronize()
    h = buf.cpu().numpy()
    outside = np.ones(len(h), bool)
    outside[offset + rows] = False
    assert_same(h[offset + rows], want, f"{what} ({A.kernel_name()})")
    assert np.isnan(h[outside]).all(), f"{what}: wrote outside its rows"


@pytest.mark.parametrize("name,kern", RB.ALL)
def test_case_bitwise(name, kern, monkeypatch):
    """every case through the kernel it was cut for, with temporal and non-temporal value loads"""
    x, want = reference(name, kern)
    for nt in (0, 1):
        K, A, S = make(name, kern, monkeypatch, nt)
        product(K, A, x, want, f"{name} {kern} nt={nt}")
        A.close()


def test_list_lengths_in_both_staging_layouts(monkeypatch):
    """the eighteen list lengths under the SKEW instantiation (rows of 16) and the plain one (rows of 15 and 17): two kernels"""
    names = set()
    for name in RB.TILE_ONLY:
        x, want = reference(name, "tile")
        K, A, S = make(name, "tile", monkeypatch, 0)
        assert S["skew"] == int(name == "lists_skew") and S["u_max"] == 2048 and min(S[f"r{k}"] for k in range(1, 9)) >= 2
        product(K, A, x, want, name)
        names.add(A.kernel_name())
        A.close()
    assert names == {"spmv_csr_tile<2048, false, true>", "spmv_csr_tile<2048, false, false>"}, names


OTHER_ENTRIES = [(name, kern) for name in ("full_blocks", "long_rows", "empty") for kern in ("stream", "tile")]


@pytest.mark.parametrize("name,kern", OTHER_ENTRIES)
def test_reversed_row_map(name, kern, monkeypatch):
    """mi_csr_create_mapped: the rows reversed into a longer y at an odd offset — every store goes through the map, every entry no row
    maps to is still NaN"""
    x, want = reference(name, kern)
    K = RB.case(name, kern)
    rowmap, ylen = RB.reversed_row_map(K.n)
    for nt in (0, 1):
        K, A, S = make(name, kern, monkeypatch, nt, rowmap=rowmap)
        product(K, A, x, want, f"{name} {kern} mapped nt={nt}", ylen=ylen, rows=rowmap.astype(np.int64))
        A.close()


@pytest.mark.parametrize("name,kern", OTHER_ENTRIES)
def test_own_stream_and_offset_views(name, kern, monkeypatch):
    """a non-blocking stream of the product's own; x and y one double into their buffers (8-byte aligned only)"""
    x, want = reference(name, kern)
    K, A, S = make(name, kern, monkeypatch, 0)
    product(K, A, x, want, f"{name} {kern} own stream", stream=torch.cuda.Stream())
    product(K, A, x, want, f"{name} {kern} offset views", offset=1)
    product(K, A, x, want, f"{name} {kern} offset views, own stream", offset=1, stream=torch.cuda.Stream())
    A.close()


@pytest.mark.parametrize("name,kern", OTHER_ENTRIES)
def test_value_refresh_on_the_device(name, kern, monkeypatch):
    """after mi_csr_update_values_dev with fresh seeded values: the new product's bits, not the old"""
    x, want = reference(name, kern)
    K, A, S = make(name, kern, monkeypatch, 0)
    product(K, A, x, want, f"{name} {kern} before")
    v = np.random.default_rng(977).uniform(-1.0, 1.0, len(K.coef))
    fresh = O.spmv(K.ptrow, K.indcol, v, x)
    assert not np.array_equal(fresh, want)
    A.update_values(dev(v))
    product(K, A, x, fresh, f"{name} {kern} refreshed")
    A.close()
