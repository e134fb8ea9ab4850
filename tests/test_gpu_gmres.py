"""mpk.GMRES on the GPU against the dense reference of tests/gmres_model.py (Arnoldi with Gram-Schmidt twice, the least-squares
problem by numpy.linalg.lstsq at every iteration: it shares neither the Givens update nor the residual recurrence it checks; its
preconditioner is the dense inverse of the MODEL's factors).

  history      every entry of the residual history, on fe:3, fe:6, chain and three random patterns, without M and with ILU(0),
               fe:6 also with ILU(1); restart 30 and restart 5 (several cycles: a restart off by one shifts every later entry)
  count        the iteration count is the reference's; len(history) == iterations + 1
  true         after convergence ||b - A x|| / ||b||, on the host in numpy.longdouble, is within 10 rtol
  exact        where the pattern drops nothing the preconditioned operator is the identity: the reference's count (1)
  csrmatrix    mult = SpMV_CSR: the same history and x, BIT for bit, as through bcsr4x4_matrix (the blocked product's chain is
               the CSR product's, and these matrices are exact 4x4 blocks)
  exits        b = 0; x0 already the solution; maxiter = restart, restart + 1, 1; restart larger than the space; NaN in b

Wall time of the file on an MI355X: 6 s."""
import numpy as np
import pytest

import bilu4_cases as C
import gmres_model as G
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

RTOL = 1e-8
FLOOR = 1e-10
# The reference's own spread: its history in float64 against its history with the Arnoldi vectors, products and dots kept in
# numpy.longdouble, over G.HISTORY_CASES x G.RESTARTS, entries above FLOOR: largest relative difference 1.56e-9 (fe:3 without M,
# restart 30, iteration 184 of 185; fe:6 without M 9.7e-10; with a preconditioner at most 2.9e-10).  Ten times it:
# (the MI355X against the float64 reference, first run: at most 5.6e-9, on fe:6 without M at restart 30; with a preconditioner 1.7e-10)
HISTORY_BOUND = 1.6e-8


def _csr(nb, bp, bc, bv):
    """The 4x4 blocks written out as CSR, every entry of every block."""
    blocks = np.asarray(bv).reshape(-1, 4, 4)
    cnt = np.repeat(4 * np.diff(bp), 4)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    col, val = [], []
    for i in range(nb):
        ks = np.arange(bp[i], bp[i + 1])
        cols = (4 * bc[ks][:, None] + np.arange(4)).reshape(-1)
        for q in range(4):
            col.append(cols)
            val.append(blocks[ks, q, :].reshape(-1))
    return ptr, np.concatenate(col).astype(np.int32), np.concatenate(val)


def _run(name, fill, b, x0=None, via="bcsr", **kw):
    """(iterations, history, x) of mpk.GMRES."""
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name) if isinstance(name, str) else name
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv) if via == "bcsr" else mpk.csrmatrix(4 * nb, *_csr(nb, bp, bc, bv))
    Mh = None if fill is None else mpk.bilu4(nb, bp, bc, bv, fill=fill)
    dx = torch.from_numpy(np.zeros(4 * nb) if x0 is None else np.array(x0, np.float64)).cuda()
    its, hist = mpk.GMRES(A, torch.from_numpy(np.ascontiguousarray(b)).cuda(), dx, M=Mh, **kw)
    x = dx.cpu().numpy()
    if Mh is not None:
        Mh.close()
    A.close()
    return its, hist, x


def _compare(label, got, ref, A, b, rtol, maxiter):
    its, hist, x = got
    rits, rhist, riter = ref
    assert len(hist) == its + 1, (label, its, len(hist))
    worst = 0.0
    for k in range(min(len(hist), len(rhist))):
        if rhist[k] > FLOOR:
            worst = max(worst, abs(hist[k] - rhist[k]) / rhist[k])
    true = G.true_residual(A, x, b)
    print(f"{label}: {its} iterations (reference {rits}), largest relative difference of the history {worst:.3e}, last {hist[-1]:.3e}, true {true:.3e}")
    assert worst <= HISTORY_BOUND, (label, worst)
    near = rtol / 2 <= rhist[-1] <= 2 * rtol
    assert its == rits or (near and abs(its - rits) == 1), (label, its, rits, rhist[-1])
    if hist[-1] <= rtol:
        assert true <= 10 * rtol, (label, true)
    else:
        assert its == maxiter, (label, its)
    return worst


@pytest.mark.parametrize("restart", G.RESTARTS)
@pytest.mark.parametrize("case", G.HISTORY_CASES, ids=lambda c: f"{c[0]}-{'none' if c[1] is None else 'ilu%d' % c[1]}")
def test_history_count_and_true_residual(case, restart):
    name, fill = case
    A, Minv, b = G.problem(name, fill)
    ref = G.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=RTOL, maxiter=300)
    got = _run(name, fill, b, restart=restart, rtol=RTOL, maxiter=300)
    _compare(f"{name} fill {fill} restart {restart}", got, ref, A, b, RTOL, 300)


@pytest.mark.parametrize("name,fill", [("chain", 0), ("chain", 2), ("fe:3", 64)])
def test_exact_factor_converges_as_the_reference_does(name, fill):
    A, Minv, b = G.problem(name, fill)
    ref = G.gmres(A, b, np.zeros_like(b), Minv, rtol=RTOL)
    got = _run(name, fill, b, rtol=RTOL)
    _compare(f"{name} fill {fill} (nothing dropped)", got, ref, A, b, RTOL, 300)
    assert got[0] == ref[0] and ref[0] <= 2, (got[0], ref[0])


@pytest.mark.parametrize("name", ["chain", "fe:6"])
@pytest.mark.parametrize("fill", [None, 0])
def test_csrmatrix_path_is_bit_equal_to_the_blocked_one(name, fill):
    A, Minv, b = G.problem(name, fill)
    blocked = _run(name, fill, b, via="bcsr", restart=5, rtol=RTOL, maxiter=40)
    csr = _run(name, fill, b, via="csr", restart=5, rtol=RTOL, maxiter=40)
    assert csr[0] == blocked[0] and (csr[0] > 5 or (name, fill) == ("chain", 0))  # more than one cycle, except where the factor is exact
    assert_bit_equal(csr[1], blocked[1], f"{name} fill {fill}: history through csrmatrix")
    assert_bit_equal(csr[2], blocked[2], f"{name} fill {fill}: x through csrmatrix")
    ref = G.gmres(A, b, np.zeros_like(b), Minv, restart=5, rtol=RTOL, maxiter=40)
    _compare(f"{name} fill {fill} through csrmatrix", csr, ref, A, b, RTOL, 40)


@pytest.mark.parametrize("fill", [None, 0])
def test_exits_without_iterating(fill):
    name = "random:31"
    A, Minv, b = G.problem(name, fill)
    n = len(b)
    its, hist, x = _run(name, fill, np.zeros(n))
    assert (its, hist) == (0, [0.0]) and not x.any()
    x0 = np.linalg.solve(A, b)
    its, hist, x = _run(name, fill, b, x0=x0)
    assert its == 0 and len(hist) == 1 and hist[0] <= 1e-14
    assert_bit_equal(x, x0, "x0 was already the solution")
    bad = b.copy()
    bad[n // 2] = np.nan
    x0 = np.arange(n) * 0.5
    its, hist, x = _run(name, fill, bad, x0=x0)
    assert its == 0 and len(hist) == 1 and np.isnan(hist[0])
    assert_bit_equal(x, x0, "NaN in b: x unchanged")


@pytest.mark.parametrize("fill", [None, 0])
@pytest.mark.parametrize("maxiter", [5, 6, 1])
def test_maxiter_at_and_around_a_restart(maxiter, fill):
    """rtol far below reach: the count is maxiter exactly, at a cycle's end (5), one iteration into the next (6) and at 1.  The
    last history entry is the recurrence's value for the x returned: it equals the true residual (rounding of the order of
    eps cond(A M^-1) apart while the residual is still of order 1e-2, as it is after at most six iterations: 1e-6 relative allowed), which fails if the last, partial cycle is not applied to x."""
    name, restart = "fe:3", 5
    A, Minv, b = G.problem(name, fill)
    ref = G.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=1e-30, maxiter=maxiter)
    got = _run(name, fill, b, restart=restart, rtol=1e-30, maxiter=maxiter)
    assert got[0] == maxiter == ref[0]
    _compare(f"{name} fill {fill} maxiter {maxiter}", got, ref, A, b, 1e-30, maxiter)
    true = G.true_residual(A, got[2], b)
    assert abs(true - got[1][-1]) <= 1e-6 * true, (true, got[1][-1])
    assert np.abs(got[2] - ref[2][-1]).max() <= 1e-6 * np.abs(ref[2][-1]).max()


def test_restart_larger_than_the_space():
    """One block (n = 4), restart 30: the Krylov space is exhausted after at most four iterations; the loop stops there with a
    finite x that solves the system, as the reference does."""
    one = C._from_rows([{0}], 91)
    A = np.asarray(one[3]).reshape(4, 4)
    b = np.array([1.0, -2.0, 0.5, 3.0])
    ref = G.gmres(A, b, np.zeros(4), restart=30, rtol=1e-13)
    its, hist, x = _run(one, None, b, restart=30, rtol=1e-13)
    assert ref[0] <= 4 and its <= 4 and len(hist) == its + 1 and abs(its - ref[0]) <= 1
    assert np.isfinite(x).all()
    assert G.true_residual(A, x, b) <= 1e-12
