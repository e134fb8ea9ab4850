"""mi_gmres_* (mpk.gmres_solver, mpk.GMRES_dev) on the GPU: a whole restart cycle enqueued on the device.

  composed     the solver against a loop written here from the library's public pieces (SpMV_BCSR / SpMV_CSR, M.solve,
               cgs(passes=2), norm2, maxpy, axpy), the two divisions in numpy on the host and the small problem of
               tests/gmres_dev_model.py: history, count, reason, fetch_cycle (hraw, y, beta) and x BIT for bit, on fe:3, chain and
               random:31, each without M, with ILU(0) exact, with sweeps(2, 2) and with sweeps(2, 2) in f32, restart 5,
               maxiter 12 (three cycles, the last one partial)
  check_every  x, history, count and reason are the same bits for check_every in {1, 2, 3, 7, restart, restart + 9}, on a solve
               that converges in the middle of a batch and on one clipped by maxiter
  reference    history within 1.6e-8 of the dense reference of tests/gmres_model.py on G.HISTORY_CASES x G.RESTARTS, its count,
               the true residual (the checks of tests/test_gpu_gmres.py)
  small        restart 1; restart 64 on random:62 (n = 136) so that step k = 63 runs; one block (n = 4) with restart 30; b = 0; x0 the
               solution; NaN in b; maxiter 1, 5, 6 at restart 5
  residual     a tridiagonal csrmatrix, n in {1, 2, 511, 513, 1025}, b and x 16-byte aligned and offset by one double, and
               n = 2 000 001 (the non-temporal path): bit-equal to the composed loop
  streams      a non-default stream gives the same bits; two solves on one handle equal two fresh handles; the read-back count;
               a capturing stream is refused with MI_ERR_STATE and stays usable
  arguments    the rules that need a handle: row counts, the kind of preconditioner, no operator

Wall time of the file on an MI355X: see profiles/NOTES.md R12.1."""
import ctypes
import functools
import math

import numpy as np
import pytest

import bilu4_cases as C
import gmres_dev_model as D
import gmres_model as G
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

RTOL = 1e-8
FLOOR = 1e-10
HISTORY_BOUND = 1.6e-8  # tests/test_gpu_gmres.py: ten times the dense reference's own spread
PRECONDS = ("none", "ilu0", "sweeps", "sweeps_f32")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _rhs(n):
    return np.sin(0.37 * np.arange(n)) + 1.0 + 0.25 * np.cos(0.011 * np.arange(n) ** 2)


def _precond(kind, mat):
    """(M as the solvers take it, the bilu4 to close)"""
    from navierstokes_amd import mpk
    if kind == "none":
        return None, None
    F = mpk.bilu4(*mat, fill=0)
    if kind == "ilu0":
        return F, F
    return F.sweeps(2, 2, precision="f32" if kind == "sweeps_f32" else "f64"), F


def composed(A, M, b, x0, restart, rtol, maxiter):
    """Restarted GMRES as include/mi355_spmv.h defines it, from the library's public pieces; the divisions by beta and by nrm in
    numpy, the small problem in tests/gmres_dev_model.py.  Returns (iterations, history, reason, x, (k, hraw, y, beta))."""
    import torch
    from navierstokes_amd import mpk
    mult = mpk.SpMV_BCSR if isinstance(A, mpk.bcsr4x4_matrix) else mpk.SpMV_CSR
    n = int(b.numel())
    x = x0.clone()
    V = torch.empty((restart + 1, n), dtype=torch.float64, device=b.device)
    w, z = torch.empty_like(b), torch.empty_like(b)
    bnorm = D.bnorm_of(float(mpk.norm2(b).item()))
    its, hist, last = 0, [], (0, np.zeros((restart, restart + 2)), np.zeros(0), 0.0)
    while True:
        mult(w, x, A)
        r = V[0]
        r.copy_(b)
        mpk.axpy(-1.0, w, r)
        beta = float(mpk.norm2(r).item())
        rel, reason = D.cycle_start(beta, bnorm, its, rtol, maxiter)
        if not hist:
            hist.append(rel)
        if reason is not None:
            return its, hist, reason, x.cpu().numpy(), (0, np.zeros((restart, restart + 2)), np.zeros(0), beta)
        with np.errstate(all="ignore"):
            r.copy_(_dev(r.cpu().numpy() / beta))
        cyc = D.Cycle(restart, beta, bnorm, rtol)
        hraw = np.zeros((restart, restart + 2))
        while cyc.k < restart and its < maxiter and not cyc.reason:
            k = cyc.k
            if M is not None:
                M.solve(z, V[k])
                mult(V[k + 1], z, A)
            else:
                mult(V[k + 1], V[k], A)
            h, nrm = mpk.cgs([V[j] for j in range(k + 1)], V[k + 1], passes=2)
            col = torch.cat([h, nrm]).cpu().numpy()
            entry = cyc.step(col)
            if entry is None:
                break
            hraw[k, : k + 2] = col
            its += 1
            hist.append(entry)
            with np.errstate(all="ignore"):
                V[k + 1].copy_(_dev(V[k + 1].cpu().numpy() / col[-1]))
        k = cyc.k
        y = np.array(cyc.solve())
        if k:
            if M is not None:
                w.zero_()
                mpk.maxpy(y, [V[j] for j in range(k)], w)
                M.solve(z, w)
                mpk.axpy(1.0, z, x)
            else:
                mpk.maxpy(y, [V[j] for j in range(k)], x)
        last = (k, hraw, y, beta)
        if cyc.reason:
            return its, hist, cyc.reason, x.cpu().numpy(), last
        if its >= maxiter:
            return its, hist, 2, x.cpu().numpy(), last


def solver_run(A, M, b, x0, restart, rtol, maxiter, check_every=5):
    """(iterations, history, reason, x, fetch_cycle(), info()) of a fresh gmres_solver."""
    import torch
    from navierstokes_amd import mpk
    S = mpk.gmres_solver(A, M, restart)
    x = x0.clone()
    its, hist, reason = S.solve(b, x, rtol=rtol, maxiter=maxiter, check_every=check_every)
    torch.cuda.synchronize()
    out = its, hist, reason, x.cpu().numpy(), S.fetch_cycle(), S.info()
    S.close()
    return out


def assert_same_solve(got, want, what):
    """history, count, reason, x and the last cycle, bit for bit; got: solver_run's, want: composed's."""
    assert (got[0], got[2]) == (want[0], want[2]), (what, got[0], got[2], want[0], want[2])
    assert len(got[1]) == got[0] + 1
    assert_bit_equal(got[1], want[1], f"{what}: history")
    assert_bit_equal(got[3], want[3], f"{what}: x")
    (k, hraw, y, beta), (wk, whraw, wy, wbeta) = got[4], want[4]
    assert k == wk, (what, k, wk)
    assert_bit_equal(hraw, whraw, f"{what}: raw columns of the last cycle")
    assert_bit_equal(y, wy, f"{what}: y of the last cycle")
    assert_bit_equal([beta], [wbeta], f"{what}: beta of the last cycle")


# ---------------------------------------------------------------- composed

@pytest.mark.parametrize("kind", PRECONDS)
@pytest.mark.parametrize("name", ["fe:3", "chain", "random:31"])
def test_bit_equal_to_the_loop_composed_from_public_pieces(name, kind):
    from navierstokes_amd import mpk
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    M, F = _precond(kind, mat)
    n = 4 * mat[0]
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = composed(A, M, b, x0, 5, 1e-30, 12)
    got = solver_run(A, M, b, x0, 5, 1e-30, 12)
    if name != "chain" or kind == "none":  # (on the chain ILU(0) is exact and the solve ends early: after 2 iterations, 10 with the sweeps)
        assert want[0] == 12 and want[2] == 2 and want[4][0] == 2  # three cycles, the last of two steps
    assert_same_solve(got, want, f"{name} {kind}")
    assert got[5]["wasted_steps_last"] == (0 if want[0] == 12 else got[5]["wasted_steps_last"]) <= 9 and got[5]["restart"] == 5
    if F is not None:
        F.close()
    A.close()


# ---------------------------------------------------------------- independence of check_every

@pytest.mark.parametrize("rtol,maxiter", [(RTOL, 300), (1e-30, 12)], ids=["converges", "maxiter"])
@pytest.mark.parametrize("kind", ["none", "sweeps"])
def test_result_does_not_depend_on_check_every(kind, rtol, maxiter):
    from navierstokes_amd import mpk
    name, restart = "random:31", 5
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    M, F = _precond(kind, mat)
    n = 4 * mat[0]
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    runs = {ce: solver_run(A, M, b, x0, restart, rtol, maxiter, check_every=ce) for ce in (1, 2, 3, 7, restart, restart + 9)}
    first = runs[1]
    assert first[2] == (1 if maxiter == 300 else 2) and (first[0] > restart or kind == "sweeps"), first[:3]  # (with the sweeps: 4 iterations)
    for ce, run in runs.items():
        assert (run[0], run[2]) == (first[0], first[2]), (ce, run[0], run[2])
        assert_bit_equal(run[1], first[1], f"check_every {ce}: history")
        assert_bit_equal(run[3], first[3], f"check_every {ce}: x")
        assert_bit_equal(run[4][1], first[4][1], f"check_every {ce}: raw columns")
        assert_bit_equal(run[4][2], first[4][2], f"check_every {ce}: y")
        info = run[5]
        cycles = -(-run[0] // restart)
        assert info["readbacks_last"] <= -(-run[0] // ce) + cycles + 1, (ce, info, run[0])
        assert 0 <= info["wasted_steps_last"] <= 2 * ce - 1, (ce, info)
        print(f"check_every {ce}: {run[0]} iterations, {info}")
    assert runs[1][5]["wasted_steps_last"] <= 1
    if F is not None:
        F.close()
    A.close()


# ---------------------------------------------------------------- the dense reference

@functools.lru_cache(maxsize=None)
def _reference(name, fill, restart):
    A, Minv, b = G.problem(name, fill)
    return A, b, G.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=RTOL, maxiter=300)


@pytest.mark.parametrize("restart", G.RESTARTS)
@pytest.mark.parametrize("case", G.HISTORY_CASES, ids=lambda c: f"{c[0]}-{'none' if c[1] is None else 'ilu%d' % c[1]}")
def test_history_count_and_true_residual_against_the_dense_reference(case, restart):
    from navierstokes_amd import mpk
    name, fill = case
    Ad, b, (rits, rhist, _) = _reference(name, fill, restart)
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    F = None if fill is None else mpk.bilu4(*mat, fill=fill)
    its, hist, reason, x, _, _ = solver_run(A, F, _dev(b), _dev(np.zeros_like(b)), restart, RTOL, 300)
    assert len(hist) == its + 1
    worst = max((abs(h - r) / r for h, r in zip(hist, rhist) if r > FLOOR), default=0.0)
    true = G.true_residual(Ad, x, b)
    print(f"{name} fill {fill} restart {restart}: {its} iterations (reference {rits}), history within {worst:.3e}, last {hist[-1]:.3e}, true {true:.3e}")
    assert worst <= HISTORY_BOUND, worst
    near = RTOL / 2 <= rhist[-1] <= 2 * RTOL
    assert its == rits or (near and abs(its - rits) == 1), (its, rits, rhist[-1])
    if hist[-1] <= RTOL:
        assert reason == 1 and true <= 10 * RTOL, (reason, true)
    else:
        assert (its, reason) == (300, 2)
    if F is not None:
        F.close()
    A.close()


# ---------------------------------------------------------------- limits of the small kernels

@pytest.mark.parametrize("name,restart,maxiter", [("chain", 1, 7), ("random:62", 64, 64)])
def test_restart_one_and_restart_sixty_four(name, restart, maxiter):
    from navierstokes_amd import mpk
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    n = 4 * mat[0]
    assert n >= restart + 1  # (random:62 has 34 block rows: n = 136)
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = composed(A, None, b, x0, restart, 1e-300, maxiter)
    got = solver_run(A, None, b, x0, restart, 1e-300, maxiter, check_every=7)
    assert want[0] == maxiter and want[4][0] == min(restart, maxiter), want[:3]  # (restart 64: step k = 63 ran)
    assert_same_solve(got, want, f"{name} restart {restart}")
    A.close()


def _one_block(seed=91):
    return C._from_rows([{0}], seed)


def test_restart_larger_than_the_space():
    """One block (n = 4), restart 30, the matrix and b of tests/test_gpu_gmres.py: at most four iterations, a finite x that solves the
    system.  With a random block the fourth direction's norm is of the order of eps, not 0: the recurrence ends the solve (reason 1)."""
    from navierstokes_amd import mpk
    one = _one_block()
    A = mpk.bcsr4x4_matrix(*one)
    Ad = np.asarray(one[3]).reshape(4, 4)
    b = np.array([1.0, -2.0, 0.5, 3.0])
    ref = G.gmres(Ad, b, np.zeros(4), restart=30, rtol=1e-13)
    its, hist, reason, x, _, _ = solver_run(A, None, _dev(b), _dev(np.zeros(4)), 30, 1e-13, 300)
    print(f"one random block: {its} iterations (reference {ref[0]}), reason {reason}, history {hist}")
    assert ref[0] <= 4 and its <= 4 and len(hist) == its + 1 and abs(its - ref[0]) <= 1
    assert reason in (1, 3) and np.isfinite(x).all()
    assert G.true_residual(Ad, x, b) <= 1e-12
    A.close()


def test_exhausted_krylov_space_is_reason_three():
    """One block (n = 4), restart 30, a Krylov space that closes EXACTLY after two steps: A maps span(e1, e2) into itself and b is a
    multiple of e1, in small integers, so that every dot and every update is exact and the third direction has norm 0.0.  By the
    definition the new g is then 0 and the history entry 0, which any rtol >= 0 reports as converged (reason 1): reason 3 is what
    a NEGATIVE rtol (never converged by the recurrence) sees.  Both are asserted; x solves the system either way."""
    from navierstokes_amd import mpk
    Ad = np.array([[2.0, 1.0, 0.0, 0.0], [4.0, 3.0, 0.0, 0.0], [0.0, 0.0, 5.0, 1.0], [0.0, 0.0, 1.0, 6.0]])
    A = mpk.bcsr4x4_matrix(1, np.array([0, 1], np.int32), np.array([0], np.int32), Ad.reshape(-1))
    b = np.array([8.0, 0.0, 0.0, 0.0])
    for rtol, expect in ((-1.0, 3), (0.0, 1), (1e-13, 1)):
        want = composed(A, None, _dev(b), _dev(np.zeros(4)), 30, rtol, 300)
        got = solver_run(A, None, _dev(b), _dev(np.zeros(4)), 30, rtol, 300)
        assert_same_solve(got, want, f"exhausted space, rtol {rtol}")
        its, hist, reason, x = got[:4]
        assert (its, reason) == (2, expect) and hist[-1] == 0.0, (rtol, its, reason, hist)
        assert got[4][1][1, 2] == 0.0  # the norm of the third direction
        assert np.isfinite(x).all() and G.true_residual(Ad, x, b) <= 1e-12
    A.close()


@pytest.mark.parametrize("kind", ["none", "ilu0"])
def test_exits_without_iterating(kind):
    from navierstokes_amd import mpk
    name = "random:31"
    mat = C.matrix(name)
    Ad, _, b = G.problem(name, None)
    n = len(b)
    A = mpk.bcsr4x4_matrix(*mat)
    M, F = _precond(kind, mat)
    its, hist, reason, x, cyc, info = solver_run(A, M, _dev(np.zeros(n)), _dev(np.zeros(n)), 30, RTOL, 300)
    assert (its, hist, reason) == (0, [0.0], 0) and not x.any() and cyc[0] == 0
    assert info["wasted_steps_last"] <= 9 and info["readbacks_last"] == 1
    x0 = np.linalg.solve(Ad, b)
    its, hist, reason, x, _, _ = solver_run(A, M, _dev(b), _dev(x0), 30, RTOL, 300)
    assert (its, reason) == (0, 0) and len(hist) == 1 and hist[0] <= 1e-14
    assert_bit_equal(x, x0, "x0 was already the solution")
    bad = b.copy()
    bad[n // 2] = np.nan
    x0 = np.arange(n) * 0.5
    its, hist, reason, x, _, _ = solver_run(A, M, _dev(bad), _dev(x0), 30, RTOL, 300)
    assert (its, reason) == (0, 4) and len(hist) == 1 and np.isnan(hist[0])
    assert_bit_equal(x, x0, "NaN in b: x unchanged")
    its, hist, reason, x, _, _ = solver_run(A, M, _dev(b), _dev(x0), 30, RTOL, 0)
    assert (its, reason) == (0, 2) and len(hist) == 1
    assert_bit_equal(x, x0, "maxiter 0: x unchanged")
    if F is not None:
        F.close()
    A.close()


@pytest.mark.parametrize("kind", ["none", "ilu0"])
@pytest.mark.parametrize("maxiter", [5, 6, 1])
def test_maxiter_at_and_around_a_restart(maxiter, kind):
    """The count is maxiter exactly, at a cycle's end (5), one iteration into the next (6) and at 1; the last history entry is the
    recurrence's value for the x returned (1e-6 relative to the true residual, as tests/test_gpu_gmres.py argues), which fails if
    the last, partial cycle is not applied to x."""
    from navierstokes_amd import mpk
    name, restart = "fe:3", 5
    mat = C.matrix(name)
    Ad, Minv, b = G.problem(name, None if kind == "none" else 0)
    A = mpk.bcsr4x4_matrix(*mat)
    M, F = _precond(kind, mat)
    ref = G.gmres(Ad, b, np.zeros_like(b), Minv, restart=restart, rtol=1e-30, maxiter=maxiter)
    want = composed(A, M, _dev(b), _dev(np.zeros_like(b)), restart, 1e-30, maxiter)
    got = solver_run(A, M, _dev(b), _dev(np.zeros_like(b)), restart, 1e-30, maxiter, check_every=2)
    assert_same_solve(got, want, f"maxiter {maxiter} {kind}")
    its, hist, reason, x = got[:4]
    assert its == maxiter == ref[0] and reason == 2
    worst = max(abs(h - r) / r for h, r in zip(hist, ref[1]))
    assert worst <= HISTORY_BOUND, worst
    true = G.true_residual(Ad, x, b)
    assert abs(true - hist[-1]) <= 1e-6 * true, (true, hist[-1])
    assert np.abs(x - ref[2][-1]).max() <= 1e-6 * np.abs(ref[2][-1]).max()
    if F is not None:
        F.close()
    A.close()


# ---------------------------------------------------------------- limits of gmres_residual

def _tridiagonal(n):
    ptr, col, val = [0], [], []
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                col.append(j)
                val.append(4.0 + 0.25 * math.sin(i) if i == j else -1.0 - 0.125 * math.cos(i + 2 * j))
        ptr.append(len(col))
    return np.array(ptr, np.int32), np.array(col, np.int32), np.array(val)


def _tridiagonal_fast(n):
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    vals = np.concatenate([-1.0 - 0.125 * np.cos(i[1:] + 2.0 * (i[1:] - 1)), 4.0 + 0.25 * np.sin(i), -1.0 - 0.125 * np.cos(i[:-1] + 2.0 * (i[:-1] + 1))])
    order = np.lexsort((cols, rows))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return ptr, cols[order].astype(np.int32), vals[order]


def _residual_case(n, offset):
    import torch
    from navierstokes_amd import mpk
    A = mpk.csrmatrix(n, *(_tridiagonal(n) if n < 5000 else _tridiagonal_fast(n)))
    bfull = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    xfull = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    b, x0 = bfull[offset: offset + n], xfull[offset: offset + n]
    assert b.data_ptr() % 16 == 8 * offset and x0.data_ptr() % 16 == 8 * offset
    b.copy_(_dev(_rhs(n)))
    x0.copy_(_dev(0.01 * np.cos(0.3 * np.arange(n))))
    want = composed(A, None, b, x0, 2, 1e-30, 2)
    got = solver_run(A, None, b, x0, 2, 1e-30, 2)
    assert_same_solve(got, want, f"tridiagonal n {n} offset {offset}")
    assert want[0] == (1 if n == 1 else 2)
    A.close()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [1, 2, 511, 513, 1025])
def test_residual_kernel_limits(n, offset):
    _residual_case(n, offset)


def test_residual_kernel_non_temporal_path():
    _residual_case(2_000_001, 0)


# ---------------------------------------------------------------- streams and reuse

def test_streams_reuse_and_capture():
    import torch
    from navierstokes_amd import mpk
    name, restart = "random:31", 5
    mat = C.matrix(name)
    n = 4 * mat[0]
    A = mpk.bcsr4x4_matrix(*mat)
    F = mpk.bilu4(*mat, fill=0)
    M = F
    b1, b2, x0 = _dev(_rhs(n)), _dev(np.cos(0.21 * np.arange(n)) - 0.5), _dev(np.zeros(n))
    fresh1 = solver_run(A, M, b1, x0, restart, RTOL, 300)
    fresh2 = solver_run(A, M, b2, x0, restart, RTOL, 300)
    assert fresh1[2] == 1 and fresh2[2] == 1 and fresh1[0] > 1
    # two solves on one handle
    S = mpk.gmres_solver(A, M, restart)
    for b, fresh in ((b1, fresh1), (b2, fresh2), (b1, fresh1)):
        x = x0.clone()
        its, hist, reason = S.solve(b, x, rtol=RTOL, maxiter=300, check_every=5)
        assert (its, reason) == (fresh[0], fresh[2])
        assert_bit_equal(hist, fresh[1], "a reused handle: history")
        assert_bit_equal(x.cpu().numpy(), fresh[3], "a reused handle: x")
        info = S.info()
        assert info["readbacks_last"] <= -(-its // 5) + -(-its // restart) + 1, info
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = x0.clone()
        its, hist, reason = S.solve(b1, x, rtol=RTOL, maxiter=300, check_every=3)
    side.synchronize()
    assert (its, reason) == (fresh1[0], fresh1[2])
    assert_bit_equal(hist, fresh1[1], "non-default stream: history")
    assert_bit_equal(x.cpu().numpy(), fresh1[3], "non-default stream: x")
    # a capturing stream: refused, nothing enqueued, the stream stays usable
    x = x0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        x.fill_(0.0)  # (so that the graph is not empty)
        with pytest.raises(mpk.MiError) as e:
            S.solve(b1, x, rtol=RTOL, maxiter=300)
    assert e.value.status == 6 and "captur" in str(e.value)
    with torch.cuda.stream(side):
        its, hist, reason = S.solve(b1, x, rtol=RTOL, maxiter=300)
    side.synchronize()
    assert (its, reason) == (fresh1[0], fresh1[2])
    assert_bit_equal(x.cpu().numpy(), fresh1[3], "after the refused capture: x")
    # host vectors: copied in and out
    xh = np.zeros(n)
    its, hist, reason = S.solve(_rhs(n), xh, rtol=RTOL, maxiter=300)
    assert (its, reason) == (fresh1[0], fresh1[2])
    assert_bit_equal(xh, fresh1[3], "host vectors: x")
    its2, hist2 = mpk.GMRES_dev(A, b1, x0.clone(), M=M, restart=restart, rtol=RTOL, maxiter=300)
    assert its2 == fresh1[0]
    assert_bit_equal(hist2, fresh1[1], "GMRES_dev: history")
    S.close()
    F.close()
    A.close()


def test_argument_rules_that_need_a_handle():
    from navierstokes_amd import mpk
    L = mpk.lib()
    mat = C.matrix("random:31")
    n = 4 * mat[0]
    A = mpk.bcsr4x4_matrix(*mat)
    other = mpk.bcsr4x4_matrix(*C.matrix("random:12"))
    F = mpk.bilu4(*C.matrix("random:12"), fill=0)
    rect = mpk.csrmatrix(2, [0, 1, 2], [0, 2], [1.0, 2.0], ncols=3)
    S = mpk.gmres_solver(A, None, 5)

    def refused(status, word, code=1):
        assert status == code, status
        assert word in L.mi_last_error().decode(), L.mi_last_error()

    refused(L.mi_gmres_set_operator_bcsr4(S.handle, other.handle), "row count")
    refused(L.mi_gmres_set_operator_csr(S.handle, rect.handle), "square")
    refused(L.mi_gmres_set_precond(S.handle, F.handle, 0, 0, 0), "row count")
    F31 = mpk.bilu4(*mat, fill=0)
    refused(L.mi_gmres_set_precond(S.handle, F31.handle, 3, 0, 0), "kind")
    refused(L.mi_gmres_set_precond(S.handle, F31.handle, 1, -1, 0), "negative")
    b, x = _dev(_rhs(n)), _dev(np.zeros(n))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    refused(L.mi_gmres_solve_dev(S.handle, None, p(x), RTOL, 10, 5, None, None, None, None), "null vector")
    refused(L.mi_gmres_solve_dev(S.handle, p(b), None, RTOL, 10, 5, None, None, None, None), "null vector")
    h = ctypes.c_void_p()
    mpk.check(L.mi_gmres_create(n, 5, ctypes.byref(h)))
    refused(L.mi_gmres_solve_dev(h, p(b), p(x), RTOL, 10, 5, None, None, None, None), "no operator", code=6)
    mpk.check(L.mi_gmres_destroy(h))
    assert not x.cpu().numpy().any()
    with pytest.raises(mpk.MiError):
        mpk.gmres_solver(A, None, 65)
    # outputs may be NULL
    mpk.check(L.mi_gmres_solve_dev(S.handle, p(b), p(x), RTOL, 3, 5, None, None, None, None))
    assert S.info()["device_bytes"] >= 8 * 8 * n
    for obj in (S, F31, F, rect, other, A):
        obj.close()
