"""The reference GMRES of tests/gmres_model.py against numpy itself, no GPU: on two small systems, with and without a
preconditioner, at a restart that forces several cycles, its final iterate is numpy.linalg.solve's, every entry of its history
from a cycle's end is the true residual of that cycle's iterate (numpy.longdouble), the iterate it returns per cycle is the one it
stopped with, and its exits (zero right-hand side, exact initial guess, maxiter, a non-finite b) count as mpk.GMRES's must."""
import numpy as np
import pytest

import gmres_model as G


@pytest.mark.parametrize("name,fill", [("random:31", None), ("random:31", 0), ("fe:3", 0), ("chain", None)])
@pytest.mark.parametrize("restart", [30, 5])
def test_reference_solves_the_system(name, fill, restart):
    A, Minv, b = G.problem(name, fill)
    rtol = 1e-12
    its, hist, iterates = G.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=rtol, maxiter=400)
    assert len(hist) == its + 1 and hist[0] == pytest.approx(1.0, rel=1e-15) and hist[-1] <= rtol
    assert len(iterates) == -(-its // restart)
    x = np.linalg.solve(A, b)
    # the residual bound turned into an error bound: |x - x*| <= cond(A) rtol |x*|
    assert np.linalg.norm(iterates[-1] - x) <= 10 * np.linalg.cond(A) * rtol * np.linalg.norm(x)
    # the least-squares residual at a cycle's end is the true residual of the iterate: rounding of the order of
    # eps cond(A M^-1) |x| / |b| apart (absolute, relative to |b|); cond < 1e4 on these diagonally dominated operators, so about 1e-12:
    # 1e-6 relative while the value is above 1e-10 leaves two orders of room
    for c, xc in enumerate(iterates):
        k = min((c + 1) * restart, its)
        true = G.true_residual(A, xc, b)
        if hist[k] > 1e-10:
            assert abs(hist[k] - true) <= 1e-6 * true, (c, hist[k], true)
        else:
            assert true <= 2e-10
    # non-increasing inside a cycle
    h = np.array(hist)
    for c0 in range(0, its, restart):
        cyc = h[c0:c0 + restart + 1]
        assert (np.diff(cyc) <= 1e-12 * cyc[:-1]).all()


def test_wide_arnoldi_agrees_with_float64():
    A, Minv, b = G.problem("random:31", 0)
    a = G.gmres(A, b, np.zeros_like(b), Minv, restart=5)
    w = G.gmres(A, b, np.zeros_like(b), Minv, restart=5, wide=True)
    assert a[0] == w[0]
    assert np.allclose(a[1], w[1], rtol=1e-8, atol=1e-10 * 1e-8)


def test_reference_exits():
    A, Minv, b = G.problem("random:31", None)
    n = len(b)
    assert G.gmres(A, np.zeros(n), np.zeros(n))[:2] == (0, [0.0])
    x = np.linalg.solve(A, b)
    its, hist, iterates = G.gmres(A, b, x)
    assert its == 0 and len(hist) == 1 and hist[0] < 1e-14 and iterates == []
    for maxiter, restart in ((5, 5), (6, 5), (1, 5)):
        its, hist, iterates = G.gmres(A, b, np.zeros(n), restart=restart, rtol=1e-30, maxiter=maxiter)
        assert its == maxiter and len(hist) == maxiter + 1 and len(iterates) == -(-maxiter // restart)
    bad = b.copy()
    bad[3] = np.nan
    its, hist, iterates = G.gmres(A, bad, np.zeros(n))
    assert its == 0 and len(hist) == 1 and np.isnan(hist[0]) and iterates == []
    # a one-block system: the space is exhausted after four iterations whatever the restart
    A4, b4 = A[:4, :4], b[:4]
    its, hist, iterates = G.gmres(A4, b4, np.zeros(4), restart=30, rtol=1e-13)
    assert its <= 4 and np.allclose(iterates[-1], np.linalg.solve(A4, b4), rtol=1e-12)
