"""spmv_csr_ring at every limit of its plan: the matrices of tests/ring_cases.py through MI_KERNEL_RING under the configuration they
were built for, BITWISE against the oracle's fma chain in CSR order (O.spmv).  No tolerance.

Every test first asserts through mi_ring_plan_census that its matrix reaches the state it is named for (tests/test_ring_limits.py
does the same on the CPU), then that the HANDLE runs that plan (ring_info, ring_shape_info, the instantiation kernel_name spells
out): a planner change that moves a case off its limit, or a silent fallback, fails the test instead of emptying it.  Every case runs
with non-temporal value loads off and on and with both staging layouts (MI355_RING_SKEW); outputs start as NaN with NaN guard
entries behind them.  Nothing here depends on a timing: MI355_SPMV_AUTOTUNE=0, MI355_PLACEMENT_DRAWS=0, MI355_REORDER=0."""
import functools
import os

import numpy as np
import pytest
import torch

import ring_cases as RC
from navierstokes_amd import mpk
from oracle import oracle as O
from test_gpu_edges import assert_same
from test_gpu_reductions import ALPHA, DATA, val
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
    for k in ("MI355_RING_DEPTH", "MI355_RING_LEAN", "MI355_RING_NT", "MI355_RING_ROW_ALIGN", "MI355_SPMV_KERNEL"):
        monkeypatch.delenv(k, raising=False)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()      # (a copy: the cases' arrays are shared and read-only)


@functools.lru_cache(maxsize=2)
def reference(name, cfg):
    """(x, y) of a case: seeded x from (-1, 1), y = the oracle's product — computed once, shared, read-only"""
    K = RC.case(name, cfg)
    x = np.random.default_rng(7000 + cfg).uniform(-1.0, 1.0, K.ncols)
    y = O.spmv(K.ptrow, K.indcol, K.coef, x)
    assert np.isfinite(y).all()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def make(name, cfg, monkeypatch, skew=0, rowmap=None, depth=None):
    """the case as a handle on the ring kernel, with what every test asserts first: the census of the case, and that the handle runs
    that plan with the instantiation asked for"""
    K = RC.case(name, cfg)
    S = mpk.ring_plan_census(K.n, K.ptrow, K.indcol, cfg)
    check_want(S, K.want, f"{name}, configuration {cfg}")
    monkeypatch.setenv("MI355_RING_CONFIG", str(cfg))
    monkeypatch.setenv("MI355_RING_SKEW", str(skew))
    if depth is not None:
        monkeypatch.setenv("MI355_RING_DEPTH", str(depth))
    A = mpk.csrmatrix(K.n, K.ptrow, K.indcol, K.coef, ncols=K.ncols, rowmap=rowmap)
    A.set_kernel("ring")
    assert A.ring_info()[:3] == (cfg, S["table_len"], S["runs_kind0"]), (A.ring_info(), S)
    shape = A.ring_shape_info()
    lean = bool(S["lean"]) and os.environ.get("MI355_RING_LEAN") != "0"
    want_depth = depth if depth is not None and cfg == 4 else S["depth"]
    assert (shape["blocks"], shape["lean"], shape["depth"]) == (S["blocks"], lean, want_depth), (shape, S)
    return K, A, S, lean, want_depth


def name_of(C, depth, mapped, nt, skew, lean):
    t = lambda b: "true" if b else "false"
    return (f"spmv_csr_ring<{C.T}, {C.NNZB}, {C.RING}, {depth}, {RC.K_RING_MAX_B}, {t(mapped)}, {t(nt)}, {t(skew)}, false, "
            f"{t(lean and C.T == 256 and depth != 3)}, false>")


def products(K, A, cfg, lean, depth, skew, want, what, mapped=False, ylen=None, rows=None, streams=(None,)):
    """y = A x with non-temporal loads off and on, on every stream given: the kernel named, the oracle's bits, NaN everywhere else"""
    x, _ = reference(*what[:2])
    ylen = K.n if ylen is None else ylen
    rows = np.arange(K.n) if rows is None else rows
    dx = dev(x)
    outside = np.ones(ylen + GUARD, bool)
    outside[rows] = False
    for nt in (0, 1):
        mpk.check(mpk.lib().mi_csr_set_nontemporal(A.handle, nt, -1))
        assert A.kernel_name() == name_of(RC.CONFIGS[cfg], depth, mapped, nt, skew, lean), A.kernel_name()
        for s in streams:
            buf = torch.full((ylen + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
            if s is None:
                mpk.SpMV_CSR(buf[:ylen], dx, A)
                torch.cuda.synchronize()
            else:
                torch.cuda.synchronize()                                 # x and buf were written on the null stream
                with torch.cuda.stream(s):
                    mpk.SpMV_CSR(buf[:ylen], dx, A)
                s.synchronize()
            h = buf.cpu().numpy()
            assert_same(h[rows], want, f"{what} nt={nt} skew={skew} stream={'null' if s is None else 'own'} ({A.kernel_name()})")
            assert np.isnan(h[outside]).all(), f"{what}: wrote outside its rows"


GPU_CASES = [(name, cfg) for name, cfg in RC.ALL if name != "r1_small"]


@pytest.mark.parametrize("name,cfg", GPU_CASES)
def test_case_bitwise(name, cfg, monkeypatch):
    """both staging layouts x both kinds of value loads; the first configuration of every case also on a stream of its own"""
    _, want = reference(name, cfg)
    own = cfg == RC.CONFIGS_OF[name][0]
    for skew in (0, 1):
        K, A, S, lean, depth = make(name, cfg, monkeypatch, skew=skew)
        streams = (None, torch.cuda.Stream()) if own and skew == 0 else (None,)
        products(K, A, cfg, lean, depth, skew, want, (name, cfg), streams=streams)
        A.close()


@pytest.mark.parametrize("name,cfg", [(nm, cfg) for nm in ("r2", "r3", "r5", "r2_rect", "r3_rect", "r5_rect") for cfg in (4, 2)])
def test_row_maps(name, cfg, monkeypatch):
    """R9: rows scattered over a longer y (the MAPPED instantiation) and rows moved up by an odd offset; every entry of y no row maps to
    is still NaN afterwards.  The rectangular forms end their last block's window at the last column."""
    _, want = reference(name, cfg)
    K = RC.case(name, cfg)
    if name.endswith("_rect"):
        assert K.ncols < K.n and int(K.indcol.max()) == K.ncols - 1
    for kind, rowmap, ylen in RC.row_maps(K.n):
        K, A, S, lean, depth = make(name, cfg, monkeypatch, skew=cfg & 1, rowmap=rowmap)
        products(K, A, cfg, lean, depth, cfg & 1, want, (name, cfg), mapped=kind == "scattered", ylen=ylen, rows=rowmap.astype(np.int64))
        A.close()


@pytest.mark.parametrize("depth", [2, 4])
def test_run_length_against_depth(depth, monkeypatch):
    """R8: runs of 1, 2, 3, 4, 5 and 9 blocks under 2 and 4 blocks of prefetch — fewer blocks than stages, and a number of blocks
    that is no multiple of the stages: the sentinel blocks behind a run"""
    _, want = reference("r8", 4)
    for skew in (0, 1):
        K, A, S, lean, d = make("r8", 4, monkeypatch, skew=skew, depth=depth)
        assert d == depth and lean and min(S[f"runs_len{k}"] for k in (1, 2, 3, 4, 5, 9)) >= 1
        products(K, A, 4, lean, depth, skew, want, ("r8", 4))
        A.close()


@pytest.mark.parametrize("name", ["r7", "r3", "r8"])
def test_general_kernel_on_a_lean_plan(name, monkeypatch):
    """R5: a LEAN-capable plan under MI355_RING_LEAN=0 runs the general configuration-4 instantiation and gives the oracle's bits —
    the bits of the LEAN instantiation (test_case_bitwise)"""
    _, want = reference(name, 4)
    monkeypatch.setenv("MI355_RING_LEAN", "0")
    K, A, S, lean, depth = make(name, 4, monkeypatch)
    assert S["lean"] == 1 and lean is False
    products(K, A, 4, False, depth, 0, want, (name, 4))


def _b_vectors(n, yo, seed):
    rng = np.random.default_rng(seed)
    for kind in ("mixed", "cancel"):
        b = DATA["mixed"](n, rng)[0]
        if kind == "cancel":                                             # b . y cancels to ~1e-12 of sum |b_i y_i|
            h = n // 2
            b[h:2 * h] = -yo[:h] * (1 + 1e-12 * rng.standard_normal(h))
            b[:h] = yo[h:2 * h]
        yield kind, b


def _dot_and_orthogonalize(A, K, x, yo, b, want, what):
    n = K.n
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    beta = mpk.SpMV_CSR_dot(y, dev(x), A, dev(b))
    assert_same(y, yo, f"{what} y")
    assert_same(np.float64(val(beta)), np.float64(want), f"{what} beta")
    x1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    x3 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    beta3 = mpk.SpMV_CSR_orthogonalize(x1, dev(x), A, dev(b), x3, ALPHA)
    assert_same(np.float64(val(beta3)), np.float64(want), f"{what} orthogonalize beta")
    assert_same(x1, yo, f"{what} x1")
    assert_same(x3, O.tree_ortho_update(ALPHA, want, b, yo), f"{what} x3")


def test_dot_epilogue_on_non_uniform_runs(monkeypatch):
    """R7 (LEAN, runs of unequal length read from run_rng, idle workgroups): the dot rides in the product's launch; beta is the model's
    tree over the layout the handle reports, and an idle workgroup's partial is 0.0"""
    x, yo = reference("r7", 4)
    K, A, S, lean, depth = make("r7", 4, monkeypatch)
    assert A.dot_in_epilogue() is True and S["uniform"] == 0 and S["runs_idle"] > 0
    layout = A.dot_epilogue_layout()
    first = layout["run_first_block"]
    assert layout["threads"] == 256 and len(first) == S["table_len"] + 1 and int(np.sum(layout["block_rows"])) == K.n
    idle = np.diff(first) == 0
    assert int(idle.sum()) == S["runs_idle"]
    for kind, b in _b_vectors(K.n, yo, 71):
        part = O.tree_ring_partials(layout, b, yo)
        assert (part[idle] == 0.0).all() and not np.signbit(part[idle]).any()
        _dot_and_orthogonalize(A, K, x, yo, b, O.tree_ring_dot(layout, b, yo), f"r7 {kind}")


@pytest.mark.parametrize("name", ["r1", "r2"])
def test_dot_behind_plans_with_plain_blocks(name, monkeypatch):
    """R1, R2 (PLAIN blocks, plain runs): rows are computed outside the counted loop, so the dot is a pass of its own: the stage-1 tree"""
    x, yo = reference(name, 4)
    K, A, S, lean, depth = make(name, 4, monkeypatch)
    assert A.dot_in_epilogue() is False and S["plain"] > 0
    with pytest.raises(mpk.MiError):
        A.dot_epilogue_layout()
    for kind, b in _b_vectors(K.n, yo, 72):
        _dot_and_orthogonalize(A, K, x, yo, b, O.tree_dot(b, yo), f"{name} {kind}")


@pytest.mark.parametrize("cfg", RC.CONFIGS_OF["r1"])
def test_value_refresh(cfg, monkeypatch):
    """R1 after mi_csr_update_values (host values) and mi_csr_update_values_dev: the plain runs and PLAIN blocks read the CSR values
    and columns, the loop reads the value stream beside its 16-bit slots — one matrix, both, the new product bit for bit"""
    x, yo = reference("r1", cfg)
    K, A, S, lean, depth = make("r1", cfg, monkeypatch)
    products(K, A, cfg, lean, depth, 0, yo, ("r1", cfg))
    for k, on_device in enumerate((False, True)):
        v = np.random.default_rng(900 + k).uniform(-1.0, 1.0, len(K.coef))
        A.update_values(dev(v) if on_device else v)
        products(K, A, cfg, lean, depth, 0, O.spmv(K.ptrow, K.indcol, v, x), ("r1", cfg))
